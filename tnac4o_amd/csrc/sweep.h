// What tn_temper (temper.hip) and tn_anneal (anneal.hip) share with tn_cell_sweep (relax.hip) and tn_cluster_exchange (exchange.hip):
// the device table of the cells, the plan of a sweep's launches, and launchers of the kernels that stay where they are.  Internal header.
#pragma once
#include <initializer_list>
#include <vector>

#include "../../include/tnpeps.h"
#include "common.h"

namespace tn {

struct SweepCell {                     // what a sweep reads of a cell (device pointers)
    const double* Es;
    const double* E1;
    const double* E4;
    const int64_t* left_map;
    const int64_t* up_map;
    int32_t q, e1cols, e4cols, staged;  // staged: the tables go to LDS
};

// the launches of one sweep over M samples: which classes of cells each colour has and the LDS their staged tables take
struct SweepPlan {
    int64_t Nx, Ny, M, ntiles, nblocks;
    std::vector<SweepCell> tab;
    int64_t lds_bytes[2][4];
    bool present[2][4];
};

// the temperature of every row (tn_temper): row m sweeps at betas[tidx[m]], a tidx outside [0, T) is read as 0; NULL betas: one beta
struct SweepBetas {
    const double* betas;
    const int32_t* tidx;
    int64_t T;
};

// relax.hip.  sweep_plan checks the cells and the grid under the name `who` (-1 and the message of tn_cell_sweep); TN_CELL_SWEEP_LDS
// is read here.  sweep_put_cells enqueues the copy of the table (it travels in kernel arguments).  sweep_once: the launches of one
// heat-bath (mode 0) or quench (mode 1) sweep, uniforms = row 0 of this sweep; rb.betas != NULL: the per-row-beta instances.
int64_t sweep_cells_bytes(int64_t Nx, int64_t Ny);
int sweep_plan(const char* who, int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, SweepPlan& plan);
int sweep_put_cells(hipStream_t st, const SweepPlan& plan, SweepCell* dev);
int sweep_once(hipStream_t st, const SweepPlan& plan, const SweepCell* dev, int16_t* states, int mode, double beta, const SweepBetas& rb,
               const double* uniforms, int64_t ldu, uint8_t* chg);
int sweep_energy(hipStream_t st, const SweepPlan& plan, const SweepCell* dev, const int16_t* states, double* energy);

// exchange.hip: the launch of tn_cluster_exchange (arguments checked by the caller; P >= 1)
int64_t cluster_exchange_max_nbits();
int cluster_exchange_launch(hipStream_t st, uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, const int32_t* rowptr, const int32_t* cols,
                            int64_t nnz, const int32_t* pairs, int64_t P, const double* uniforms, int32_t* size_out, int32_t* diff_out);

// temper.hip: states -> packed spin bits of tn_temper (rows: M x ceil(nbits / 64) words, every word written; M x words / 256 below 2^31 is
// the caller's duty), the one source of the conversion for tn_ladder_measure (ladder.hip) too
int temper_to_bits_launch(hipStream_t st, const SweepCell* cells, const int16_t* states, int64_t ncell, int64_t M, int64_t nbits, const int32_t* bitcell,
                          uint64_t* rows);

// the product of non-negative factors fits an index: no overflow and below 2^60
inline bool mul_fits(std::initializer_list<int64_t> f) {
    int64_t p = 1;
    for (int64_t x : f)
        if (x < 0 || __builtin_mul_overflow(p, x, &p)) return false;
    return p < ((int64_t)1 << 60);
}

}  // namespace tn
