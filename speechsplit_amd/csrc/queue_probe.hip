// Hardware-queue probe behind ss_bind: picks the engine's three branch streams by measuring which candidates share a hardware queue.
#include <cstdio>
#include <string>
#include <vector>

#include "abi.h"
#include "kernels.h"

namespace ss {

namespace {

// ---- hardware-queue probe ---------------------------------------------------------------------------------------------------------
// HIP multiplexes a process's streams onto a few in-order hardware queues (4 by default) and does not say which stream got which.
// Two streams on one queue execute strictly one after the other, so the step's branches lose the concurrency they exist for:
// measured 6.34 ms with the four engine streams on four queues against 7.22 ms with the side stream on the main stream's queue
// (profiles/r02/stream_order_effect.txt; which case one gets depends on how many streams the process -- PyTorch, RCCL -- created
// before).  The serialisation is also what makes the assignment MEASURABLE: a kernel that spins for ~400 us on stream A delays a
// trivial kernel on stream B only if A and B share a queue.
__global__ void queue_probe_spin_kernel(long long ticks) {      // wall_clock64: constant 100 MHz
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
__global__ void queue_probe_nop_kernel() {}

// true if a and b are served by the same hardware queue
bool same_queue(hipStream_t a, hipStream_t b, hipEvent_t ea, hipEvent_t eb0, hipEvent_t eb1) {
    constexpr long long SPIN_TICKS = 40000;                       // 400 us
    (void)hipStreamSynchronize(a);
    (void)hipStreamSynchronize(b);
    hipLaunchKernelGGL(queue_probe_spin_kernel, dim3(1), dim3(1), 0, a, SPIN_TICKS);
    (void)hipEventRecord(ea, a);
    (void)hipEventRecord(eb0, b);
    hipLaunchKernelGGL(queue_probe_nop_kernel, dim3(1), dim3(1), 0, b);
    (void)hipEventRecord(eb1, b);
    // poll (a blocking wait may wake up later than the spin lasts): b's kernel finished -- had a's spin finished by then?  On separate
    // queues b is done after a few microseconds and the spin is not.
    bool spin_done = false;
    for (long polls = 0;; ++polls) {
        const bool a_done = hipEventQuery(ea) == hipSuccess;
        if (hipEventQuery(eb1) == hipSuccess) {
            spin_done = a_done;
            break;
        }
        if (a_done || polls > 20000000L) {              // the spin ended first: b was held up behind it (or the device does not answer: count it as shared)
            spin_done = true;
            break;
        }
    }
    (void)hipStreamSynchronize(a);
    return spin_done;
}
// the same measurement, repeated when it says "shared": a co-tenant of the GPU that delays stream b for the length of the spin makes separate
// queues look shared once; it does not do so three times in a row
bool same_queue_voted(hipStream_t a, hipStream_t b, hipEvent_t ea, hipEvent_t eb0, hipEvent_t eb1) {
    for (int i = 0; i < 3; ++i)
        if (!same_queue(a, b, ea, eb0, eb1)) return false;
    return true;
}

}  // namespace

// Choose three branch streams from a pool of fresh streams so that they and `main` sit on four different hardware queues
// (as far as the device's queue count allows); the rest of the pool is destroyed.
int pick_streams(hipStream_t main, hipStream_t branch[3], std::string& report) {
    constexpr int POOL = 10;
    struct Guard {               // whatever is still in here when the function returns -- early on an error, or at its end -- is destroyed
        hipStream_t pool[POOL] = {};
        hipEvent_t ev[3] = {};
        ~Guard() {
            for (auto& st : pool)
                if (st) (void)hipStreamDestroy(st);
            for (auto& x : ev)
                if (x) (void)hipEventDestroy(x);
        }
    } gd;
    hipStream_t(&pool)[POOL] = gd.pool;
    hipEvent_t(&ev)[3] = gd.ev;
    for (auto& x : ev) HIPCHK(hipEventCreateWithFlags(&x, hipEventDisableTiming));
    for (auto& st : pool) {
        HIPCHK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, 0));      // (created with the lowest priority instead: measured 5.78 vs 5.80 ms, not done)
        hipLaunchKernelGGL(queue_probe_nop_kernel, dim3(1), dim3(1), 0, st);      // first use of a stream sets its queue up: not inside a measurement
    }
    hipLaunchKernelGGL(queue_probe_nop_kernel, dim3(1), dim3(1), 0, main);
    HIPCHK(hipDeviceSynchronize());
    std::vector<hipStream_t> chosen;
    char buf[64];
    report.clear();
    for (int pass = 0; pass < 2 && chosen.size() < 3; ++pass)       // pass 1: accept streams that only differ from the main stream's queue
        for (int i = 0; i < POOL && chosen.size() < 3; ++i) {
            if (!pool[i]) continue;
            bool clash = same_queue_voted(main, pool[i], ev[0], ev[1], ev[2]);
            for (size_t k = 0; k < chosen.size() && !clash && pass == 0; ++k) clash = same_queue_voted(chosen[k], pool[i], ev[0], ev[1], ev[2]);
            if (!clash) {
                std::snprintf(buf, sizeof buf, "%scandidate %d%s", chosen.empty() ? "" : ", ", i, pass ? " (shares a queue with another branch)" : "");
                report += buf;
                chosen.push_back(pool[i]);
                pool[i] = nullptr;
            }
        }
    for (int i = 0; i < POOL && chosen.size() < 3; ++i)             // a device with fewer queues than streams: take what is there
        if (pool[i]) {
            chosen.push_back(pool[i]);
            pool[i] = nullptr;
            report += " +fallback";
        }
    branch[0] = chosen[0];
    branch[1] = chosen[1];
    branch[2] = chosen[2];
    report = "branch streams on hardware queues of their own: " + report;
    return 0;
}

}  // namespace ss
