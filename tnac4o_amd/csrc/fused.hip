// Host side of the launches with in-kernel barriers: cq_fused_kernel (cholqr.hip), sq_kernel (smallqr.hip), svdl_kernel (small.hip).
// What the three share: a slot per stream (statistics, barrier state), the co-residency budget their grids must respect, the admission
// of tall panels, the environment switches of the barriers, and the check for launches that gave up.
#include <stdlib.h>

#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "common.h"

namespace tn {

// TN_PANEL_FUSED=0 keeps the six-launch chain for every panel (A/B measurements, cross-checks); read per call: the tests switch it
static bool cq_fused_enabled() { return env_flag_on("TN_PANEL_FUSED"); }

unsigned panel_spin_limit() { return (unsigned)env_i64("TN_PANEL_SPIN_LIMIT", CQ_SPIN_LIMIT); }
int panel_maxpass() {
    static const int maxpass = [] { const int v = env_int("TN_PANEL_MAXPASS", CQ_MAXPASS); return v >= 1 && v <= CQ_MAXPASS ? v : CQ_MAXPASS; }();
    return maxpass;
}

void* device_pool_slot(const void* symbol, size_t slot_bytes, int slot) {
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, char*> bases;      // a __device__ symbol has one address per device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) { (void)hipGetLastError(); return nullptr; }
    std::lock_guard<std::mutex> lk(mu);
    char*& base = bases[std::make_pair(symbol, dev)];
    if (!base) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, symbol) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        base = (char*)p;
    }
    return base + (size_t)slot * slot_bytes;
}

// slot of a stream (first come, first served; the streams beyond CHOLQR_SLOTS share the last slot)
static std::mutex cq_slot_mu;
static std::map<hipStream_t, int> cq_slot_of;
static std::vector<int> cq_slot_free;                               // slots of destroyed streams (tn_stream_destroy), handed out again first
static int cq_slot_next = 0;
int cholqr_stream_slot(hipStream_t st) {
    std::lock_guard<std::mutex> lk(cq_slot_mu);
    auto it = cq_slot_of.find(st);
    if (it != cq_slot_of.end()) return it->second;
    int s = CHOLQR_SLOTS;
    if (!cq_slot_free.empty()) { s = cq_slot_free.back(); cq_slot_free.pop_back(); }
    else if (cq_slot_next < CHOLQR_SLOTS) s = cq_slot_next++;
    cq_slot_of.emplace(st, s);
    return s;
}

// Co-residency budget of the launches with in-kernel barriers: a workgroup of them
// needs a whole CU and waits only for workgroups of its own launch, so launches in flight cannot deadlock while together they ask
// for no more CUs than this process may count on.  Nothing about that is assumed: the budget is derived at first use from
//   * the device (hipDeviceAttributeMultiprocessorCount), or TN_PANEL_CU_BUDGET when several processes share the card (the CUs this
//     process may count on: half the chip for two tenants ...; 0 keeps every panel on the six-launch chain),
//   * the number of hardware queues the runtime multiplexes the streams onto (GPU_MAX_HW_QUEUES as the runtime itself reads it at
//     initialisation; 4 when unset): at most that many kernels of the process are in flight,
// which gives  maxblk = min(32, budget / queues)  workgroups for an ordinary launch (32 with the package's 8 queues on an MI355X).  A
// taller panel (up to 2 maxblk workgroups) is admitted only while the budget still holds with it:
//     2 maxblk B + maxblk (S - B) <= budget,   S = min(streams of this process that have run panels, queues),  B = tall launches in
// flight (this one included): all four chains of a solve when nothing else runs panels, three with a fifth stream around, none with
// eight.  In-flight tall launches are tracked with one event per stream (recorded behind the launch, queried before the next
// admission, all under one mutex that also covers the launch itself).  Streams created with a CU mask (tn_stream_create_masked) and
// streams on which a launch has ever given up at a barrier (fused_timeouts) are taken off these forms for good.  A panel that is not
// admitted takes the six-launch chain: the result is the same bit for bit.  TN_PANEL_FUSED_BIG=0: never admit tall panels.
struct FusedBudget { int cus = 0, queues = 4, maxblk = 0; bool ready = false; };
static FusedBudget cq_budget_of[16];
static std::mutex cq_budget_mu;
static FusedBudget fused_budget() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) { (void)hipGetLastError(); return FusedBudget(); }
    std::lock_guard<std::mutex> lk(cq_budget_mu);
    FusedBudget& b = cq_budget_of[dev];
    if (!b.ready) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) { (void)hipGetLastError(); cus = 0; }
        const int budget = env_int("TN_PANEL_CU_BUDGET", -1);
        if (budget >= 0 && budget < cus) cus = budget;
        const int hwq = env_int("GPU_MAX_HW_QUEUES", 4), q = hwq >= 1 ? hwq : 4;
        b.cus = cus; b.queues = q;
        b.maxblk = cus / q < CQ_FUSED_MAXBLK ? cus / q : CQ_FUSED_MAXBLK;
        b.ready = true;
    }
    return b;
}
int fused_maxblk() { return fused_budget().maxblk; }
static std::map<hipStream_t, bool> cq_stream_off;                  // (guarded by cq_slot_mu)
void fused_forms_disable(hipStream_t st) {
    std::lock_guard<std::mutex> lk(cq_slot_mu);
    cq_stream_off[st] = true;
}
// tn_stream_destroy: the stream's slot (statistics, panel state, admission bookkeeping) goes back to the pool, so that the count of
// live streams the admission of tall panels works with stays a count of LIVE streams
void fused_stream_released(hipStream_t st) {
    std::lock_guard<std::mutex> lk(cq_slot_mu);
    cq_stream_off.erase(st);
    auto it = cq_slot_of.find(st);
    if (it == cq_slot_of.end()) return;
    const int slot = it->second;
    cq_slot_of.erase(it);
    if (slot < CHOLQR_SLOTS) { cq_slot_free.push_back(slot); cholqr_state_dirty(slot); }
}
static bool cq_stream_is_off(hipStream_t st) {
    std::lock_guard<std::mutex> lk(cq_slot_mu);
    return cq_stream_off.count(st) != 0;
}
// may a launch of nwg workgroups with in-kernel barriers go out on this stream?
bool fused_forms_allowed(hipStream_t st, int nwg) {
    if (!cq_fused_enabled() || cq_stream_is_off(st)) return false;
    if (cholqr_stream_slot(st) >= CHOLQR_SLOTS) return false;
    return nwg <= fused_budget().maxblk;
}

struct CqBigTrack {
    hipEvent_t ev[CHOLQR_SLOTS + 1] = {};
    bool pending[CHOLQR_SLOTS + 1] = {};
};
static CqBigTrack cq_big;
static std::mutex cq_big_mu;
static bool cq_big_enabled() { return env_flag_on("TN_PANEL_FUSED_BIG"); }      // read per call: the tests switch it
// call with cq_big_mu held
static bool cq_big_admit(int slot, int nslots) {
    if (slot >= CHOLQR_SLOTS) return false;                        // streams without a slot of their own are not tracked
    const FusedBudget b = fused_budget();
    if (b.maxblk < 1) return false;
    int inflight = 0;
    for (int s = 0; s < CHOLQR_SLOTS; ++s) {
        if (s == slot || !cq_big.pending[s]) continue;            // (an earlier tall launch of THIS stream is not concurrent with the new one)
        if (hipEventQuery(cq_big.ev[s]) == hipSuccess) cq_big.pending[s] = false;
        else ++inflight;
    }
    const int S = nslots < b.queues ? nslots : b.queues;
    return inflight + 1 <= b.cus / b.maxblk - S;
}
FusedTallLaunch::FusedTallLaunch(hipStream_t st, bool wanted) : st_(st), slot_(wanted ? cholqr_stream_slot(st) : CHOLQR_SLOTS) {
    if (!wanted || !cq_big_enabled()) return;
    int nslots;
    { std::lock_guard<std::mutex> lk(cq_slot_mu); nslots = (int)cq_slot_of.size(); }
    cq_big_mu.lock();
    admitted = cq_big_admit(slot_, nslots);
    if (!admitted) cq_big_mu.unlock();
}
void FusedTallLaunch::release() {
    if (admitted) { admitted = false; cq_big_mu.unlock(); }
}
FusedTallLaunch::~FusedTallLaunch() { release(); }
void FusedTallLaunch::launched() {
    if (!admitted) return;
    if (!cq_big.ev[slot_] && hipEventCreateWithFlags(&cq_big.ev[slot_], hipEventDisableTiming) != hipSuccess) cq_big.ev[slot_] = nullptr;
    else if (hipEventRecord(cq_big.ev[slot_], st_) == hipSuccess) cq_big.pending[slot_] = true;
    release();
}

// ---- time-outs of the launches with in-kernel barriers ----------------------------------------------------------------------
// A launch that gives up at a barrier poisons its outputs with NaN and adds to a sticky per-stream device counter (cq_stats[10]
// in cholqr.hip, sq_stats[3] in smallqr.hip).  Every caller that has enqueued such launches asks fused_timeouts before it hands results
// back: one 16-byte read-back and a synchronisation.  A positive answer means: the results of the stream since the previous
// check are invalid, the stream has been taken off the single-launch forms (the co-residency the spins rely on evidently does
// not hold: another tenant on the card, a debugger, ...), its barrier state is cleared, and the caller must redo the work -- which
// now takes the six-launch chain / the blocked path, bit-identical results.  Callers that own many factorisations (tn_compress_mps)
// defer the check to the end of their call (FusedDeferCheck).
static thread_local long cq_fused_launches = 0;                    // launches with in-kernel barriers enqueued by this thread since its last check
static thread_local int cq_defer_depth = 0;
void fused_note_launch() { ++cq_fused_launches; }
void fused_defer_push() { ++cq_defer_depth; }
void fused_defer_pop() { --cq_defer_depth; }
bool fused_check_deferred() { return cq_defer_depth > 0; }
bool fused_check_needed() { return cq_fused_launches > 0; }
static unsigned long long cq_timeouts_seen[CHOLQR_SLOTS + 1][2];   // last values of the two counters per slot (guarded by cq_slot_mu)
int fused_timeouts(hipStream_t st, int* count_out) {
    *count_out = 0;
    cq_fused_launches = 0;
    const int slot = cholqr_stream_slot(st);
    if (slot >= CHOLQR_SLOTS) return 0;                            // such streams never take these forms
    unsigned long long a;
    int rc = cholqr_gaveup_count(st, slot, &a);
    if (rc) return rc;
    unsigned long long sq[4];
    rc = smallqr_stats(st, sq, 0);
    if (rc) return rc;
    unsigned long long da, db;
    {
        std::lock_guard<std::mutex> lk(cq_slot_mu);
        da = a - cq_timeouts_seen[slot][0];
        db = sq[3] - cq_timeouts_seen[slot][1];
        cq_timeouts_seen[slot][0] = a;
        cq_timeouts_seen[slot][1] = sq[3];
        if (da + db > 0) cq_stream_off[st] = true;
    }
    if (da + db == 0) return 0;
    *count_out = (int)(da + db > 2147483647ull ? 2147483647ull : da + db);
    fprintf(stderr, "[libtnpeps] %llu launch(es) with in-kernel barriers gave up on stream %p (workgroups not co-resident: is the device shared? "
            "see TN_PANEL_CU_BUDGET); the work is redone through the multi-launch forms, which this stream uses from now on\n",
            (unsigned long long)(da + db), (void*)st);
    // leave a clean slate: the stream's panel state (sticky flag, barrier counter) and the small-QR barrier state
    {
        std::lock_guard<std::mutex> lk(cq_slot_mu);
        cholqr_state_dirty(slot);
    }
    if ((rc = smallqr_reset_state(st))) return rc;
    return 0;
}

}  // namespace tn
