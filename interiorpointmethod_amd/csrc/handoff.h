// handoff.h -- the ONE statement of the device-side hand-off protocol: how a workgroup passes data to workgroups on other CUs,
// XCDs and streams through a counter or flag word, without a stream event or a launch boundary (gfx950).
//
// The protocol (agent-scope release / acquire; kernel guide: Guideline 16 and Pitfall 12 of cdna_hip_programming.md,
// MI355X_MICROARCH.md "inter-workgroup visibility"):
//   producer   plain stores; EVERY storing wave drains them (s_waitcnt vmcnt(0)); the workgroup meets; lane 0 issues the agent-scope
//              release (L2 write-back), WAITS FOR IT (the second s_waitcnt vmcnt(0): without it the signal below may pass the
//              write-back), and only then bumps the counter / stores the flag with a relaxed agent-scope atomic
//              -> handoff_publish_begin(), then the caller's own signal on lane 0
//   consumer   one lane (the sparse sweeps: the lanes of wave 0) polls the word relaxed, BOUNDED; then that lane's agent-scope acquire
//              (invalidates this CU's L1 for the whole workgroup) and its wait; then the workgroup barrier; then plain loads
//              -> handoff_wait / handoff_wait_ge, handoff_acquire, __syncthreads() (handoff_acquire_barrier does the last two)
//   skipped    a producer launch that finds the `done` latch set still signals -> handoff_skipped
// Every spin is bounded by ipm_spin_limit: a wait that runs into it sets the handle's time-out word, which releases every other
// waiter of the call at its next look (every 1024th poll); the host rolls the call back and repeats it on a path that does not poll.
// The tests do NOT catch a missing acquire or a lost second wait: this file is where they are reviewed.
#pragma once
#include <hip/hip_runtime.h>

namespace ipm {

// Bound of every device-side hand-off spin (polls of ~0.2 us: about 0.7 s).  TEST KNOB: the environment variable
// IPM_TEST_SPIN_LIMIT (read at ipm_create) lowers it so that the recovery paths can be driven on purpose (tests only).
__device__ unsigned ipm_spin_limit = 1u << 22;

// Diagnostic record (optional, 8 words, zeroed by the host): the FIRST wait that ran into the bound writes
// {1, tag, kind, target, seen}; HD_COUNT goes on counting the waits that gave up after it.
enum { HD_COUNT = 0, HD_TAG, HD_KIND, HD_TARGET, HD_SEEN, HD_WORDS = 8 };
// kind = which wait it was.  The kinds below HK_ROLES are the waits of the fused launch's WORKERS (tag = index of the work item);
// from HK_ROLES on the waiter is a chain role of that launch or a kernel of the serial path (tag = step, see the call sites).
enum HandoffKind : unsigned {
    HK_FCOUNT = 1,          // worker: the formation chunks of its tile
    HK_TPROG = 2,           // worker: the previous update item of its tile
    HK_LFINAL_ROW = 3,      // worker: L of its tile's row, columns [j0, j1)
    HK_LFINAL_COL = 4,      // worker: the same of its tile's column
    HK_POTRFDONE = 5,       // worker: the diagonal block of its panel solve
    HK_ROLES = 6,
    HK_GEMM = 6,            // gemm_nt_f64_kernel's wait_on, and the critical products of the fused launch (ff_crit_role)
    HK_POTRF = 7,           // potrf_diag_body's wait_on (serial path and the chain role)
    HK_DCOUNT = 8,          // the chain role: max diag(B) complete
};

__device__ __forceinline__ unsigned handoff_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The bounded wait, called by the polling lane(s) only: polls ready() with s_sleep SLEEP between two polls until it holds (-> true)
// or the wait gives up (-> false): past ipm_spin_limit polls, or at once when another wait of the call already gave up.  In the
// first case the first wait to give up claims the diagnostic record (dbg, may be null) and fills it with record(), BEFORE the
// time-out word releases the other waiters.  NULL_OK: `timeout` may be null (the wait is then bounded all the same, and silent).
// HandoffSink: where a wait that gives up reports (the time-out word, the record).  One small aggregate by value on purpose: as two
// pointer parameters the null tests compile to other instructions in every caller (profiles/handoff_isa_parent_vs_this.txt).
struct HandoffSink { unsigned* timeout; unsigned* dbg; };
template <int SLEEP, bool NULL_OK, class Ready, class Record>
__device__ __forceinline__ bool handoff_wait(Ready ready, HandoffSink sink, Record record) {
    unsigned* const timeout = sink.timeout; unsigned* const dbg = sink.dbg;
    unsigned spins = 0;
    bool ok = true;
    while (!ready()) {
        __builtin_amdgcn_s_sleep(SLEEP);
        ++spins;
        if (spins > ipm_spin_limit || ((spins & 1023u) == 1u && (!NULL_OK || timeout) && handoff_load(timeout))) {
            if (spins > ipm_spin_limit && dbg && __hip_atomic_fetch_add(dbg + HD_COUNT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) record();
            if (!NULL_OK || timeout) __hip_atomic_store(timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = false;
            break;
        }
    }
    return ok;
}

// The record of a wait for *p >= target (HD_COUNT is the claim, taken by handoff_wait)
__device__ __forceinline__ void handoff_record_ge(unsigned* dbg, unsigned tag, unsigned kind, unsigned target, const unsigned* p) {
    dbg[HD_TAG] = tag; dbg[HD_KIND] = kind; dbg[HD_TARGET] = target; dbg[HD_SEEN] = handoff_load(p);
}

// The common wait: *p >= count, with the record (dbg may be null).
template <int SLEEP, bool NULL_OK>
__device__ __forceinline__ bool handoff_wait_ge(const unsigned* p, unsigned count, HandoffSink sink, unsigned tag, unsigned kind) {
    return handoff_wait<SLEEP, NULL_OK>([=] { return handoff_load(p) >= count; }, sink, [=] { handoff_record_ge(sink.dbg, tag, kind, count, p); });
}

// Consumer, behind its wait(s): the polling lane's (wave's) acquire and its wait.  The workgroup barrier follows.
template <bool WAIT = true>
__device__ __forceinline__ void handoff_acquire() {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (WAIT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (WAIT = false: ff_gate_kernel, which ends behind its acquire)
}
__device__ __forceinline__ void handoff_acquire_barrier(bool polled) {       // polled: this thread belongs to the lane / wave that waited
    if (polled) handoff_acquire();
    __syncthreads();
}

// Producer, behind its last store, called by the WHOLE workgroup: drain, barrier, lane 0's release and its wait.  Lane 0 then
// signals:  handoff_publish_begin(); if (threadIdx.x == 0) <counter add(s) / flag store, relaxed, agent scope>;
__device__ __forceinline__ void handoff_publish_begin() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every storing wave drains its stores
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the write-back is complete before the signal goes out
    }
}

// A skipped producer still signals: the stop test may flip `done` while a factorization is in flight (it runs on the residual
// stream), and a consumer that passed its own check must not spin on a counter nobody bumps.  True: skipped, the caller returns.
__device__ __forceinline__ bool handoff_skipped(const int* done, unsigned* signal) {
    if (done && *done) {
        if (signal && threadIdx.x == 0) __hip_atomic_fetch_add(signal, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return true;
    }
    return false;
}

// Progress signal at the ENTRY of a kernel, for the stores of the kernel IN FRONT of it in the same stream: that kernel has ended,
// and a kernel's end releases its stores at agent scope, so nothing is drained or fenced here -- the first lane of the first workgroup
// stores the word, relaxed.  `value` is the host's epoch count (monotone over the handle's life: the word is never cleared and a
// roll-back needs no repair).  Called BEFORE the kernel's test of the `done` latch: like handoff_skipped, a kernel that finds the
// latch set still signals.  The consumer is ff_gate_kernel on another stream (host_iteration.h, the streamed A^T dy pieces).
__device__ __forceinline__ void handoff_signal_at_entry(unsigned* word, unsigned value) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) __hip_atomic_store(word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace ipm
