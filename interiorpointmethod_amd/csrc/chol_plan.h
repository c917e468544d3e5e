// chol_plan.h -- the STEP PLAN of the dense blocked Cholesky (host_factor_solve.h: enqueue_factor walks it and decides nothing).
// Plain host code over integers: built into libipm_hip.so and checked on the CPU through ipm_debug_chol_plan
// (tests/test_chol_plan_host.py replays every plan against the dependency rules of the factorization).
//
// Right-looking, one step per 128-row block column k, with one step of look-ahead on two streams:
//   main stream : potrf_diag(k) -> [wait bulk(k-1)] -> panel rows of block k+1 -> update of tile (k+1,k+1)
//   bulk stream : [wait crit(k)] panel rows >= k+2 -> rest of the trailing update
// so the serial diagonal-block factorization of step k+1 overlaps the bulk update of step k.  Without look-ahead (batched mode,
// small handles) panel and update of a step follow each other on the one stream.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "gemm_nt_f64.h"
#include "potrf_f64.h"

namespace ipm {

enum { CS_NARROW = 0, CS_WIDE = 1, CS_LOOKAHEAD = 2 };         // CholStep::shape
enum { CH_NONE = 0, CH_COUNTER = 1, CH_EVENT = 2 };            // a hand-off: none, a device counter that is polled, a stream event

struct CholStep {
    int potrf_panels, rows;       // potrf_diag(k): 16-wide panels it factors, rows of the LP in block k (<= 0: padding only)
    int rem;                      // rows below the diagonal block after the envelope clip; 0: no panel and no update in this column
    int shape;                    // CS_NARROW / CS_WIDE: single-stream tile shapes; CS_LOOKAHEAD: critical part + bulk part
    int g0, gend;                 // the step's group of the two-level schedule: block columns [g0, gend)
    int kcols;                    // block columns the trailing update applies: 1, or k - g0 + 1 (the deferred update, K = 128 kcols)
    int window;                   // > 0: the bulk update is the window of this many block columns from k+1 on, the rest is deferred
    int crit_wait, crit_count;    // the critical panel waits for the bulk update of step k-1: CH_NONE, counter k-1 >= crit_count, event k-1
    int crit_flag, poll_count;    // 1: the critical panel signals counter nblk+k, the bulk panel polls it for poll_count workgroups (else event k)
    int bulk, bulk_count;         // bulk update: CH_NONE (none), CH_COUNTER (signals counter k: bulk_count workgroups), CH_EVENT
    int bulk_event;               // 1: the bulk stream records event k when the step is enqueued
};
constexpr int CHOL_STEP_WORDS = (int)(sizeof(CholStep) / sizeof(int));

struct CholPlan {
    int lookahead, polling;                       // two streams; device counters in use (cleared before the first step)
    int gs, n_counter_steps, n_event_steps;       // what ipm_get_schedule reports
    std::vector<CholStep> steps;                  // one per block column
};

// la: look-ahead on two streams; fs: hand-offs may be device-polled counters (only while this is the one live handle on the device);
// shift: a Tikhonov shift is in effect; env_last: tile envelope (rows below block env_last[k] of column k are zero and stay zero) or null.
inline CholPlan chol_step_plan(int nblk, int64_t m, int64_t mp, bool la, bool fs, int two_level, int group_steps, int ss_small_blocks,
                               bool shift, const int* env_last) {
    CholPlan p{la, la && fs, 1, 0, 0, std::vector<CholStep>((size_t)nblk, CholStep{})};
    // group size of the two-level schedule.  Measured (factor, ms): 16384 x 32768: 39.7 / 34.9 / 33.4 / 32.9 / 32.5 for groups
    // of 1 / 2 / 3 / 4 / 6; 8192 x 16384: 7.87 / 7.46 / 7.34 / 7.34 for 1 / 2 / 3 / 4; but 4096 x 8192: 2.21 -> 2.36 with groups
    // of 2 (half of its steps are bound by the pivot chain, which grouping lengthens): on from 48 blocks.
    // IPM_TWO_LEVEL=0 disables, IPM_GROUP_STEPS=n forces a group size (>= 8 blocks).
    if (la && !env_last && two_level != 0) {
        if (group_steps > 0) p.gs = nblk >= 8 ? group_steps : 1;
        else if (nblk >= 96) p.gs = 4;
        else if (nblk >= 48) p.gs = 3;
    }
    for (int k = 0; k < nblk; ++k) {
        CholStep& s = p.steps[k];
        // 16-wide panels of diagonal block k that hold rows of the LP (the rest of the block is padding: unit diagonal): potrf_diag
        // factors only those -- the last real block of an LP whose row count is no multiple of 128, and the blocks the layout pads
        // with.  (The Tikhonov shift touches every diagonal entry: keep the full block.)
        const int64_t real = m - (int64_t)k * NB;
        s.potrf_panels = shift || real >= NB ? NB / 16 : (int)std::max<int64_t>(1, (real + 15) / 16);
        s.rows = (int)real;
        // Group table: uniform groups of gs block columns (from 48 blocks on; one-level below that -- pairing only the head of the
        // factorization was measured and does not pay below 48 blocks either: 2.158 / 2.157 / 2.182 / 2.213 ms for 0 / 4 / 8 / 16 paired steps)
        s.g0 = p.gs > 1 ? (k / p.gs) * p.gs : k;
        s.gend = p.gs > 1 ? std::min(s.g0 + p.gs, nblk) : k + 1;
        s.kcols = 1;
        s.rem = (int)(mp - (int64_t)(k + 1) * NB);
        if (env_last) s.rem = std::max(0, std::min(s.rem, (env_last[k] - k) * NB));      // rows below the envelope are zero and stay zero
        // one stream (batched mode, small handles): panel and update are BOTH on the dependent chain of the step.  With few
        // trailing blocks the chip is empty anyway: narrower tiles (32-row panel strips on 8 waves / 64 x 64 update tiles) are
        // latency-shorter kernels -- ss_small_blocks = trailing blocks up to which they are used (16, or every step of a
        // lockstep handle: fixed by ipm_create, no environment switch reads it)
        s.shape = la ? CS_LOOKAHEAD : s.rem <= ss_small_blocks * NB ? CS_NARROW : CS_WIDE;
        s.bulk_event = la && k + 1 < nblk;
        if (!la || s.rem <= 0) continue;                            // (look-ahead, nothing below the diagonal block: only the event)
        // the previous bulk update either signalled a counter (small grids) or recorded an event
        if (k >= 1) { s.crit_wait = p.steps[k - 1].bulk == CH_COUNTER ? CH_COUNTER : CH_EVENT; s.crit_count = p.steps[k - 1].bulk_count; }
        // bulk side: the (small) panel launch of the bulk stream polls the completion counter of the critical
        // panel launch instead of a stream event, unless it is large enough to crowd the CUs while it spins
        const int tb_wgs = gemm_tiles(s.rem - NB, NB, 64, 128, 0, 0);
        // SAFETY: a polling launch holds LDS on every CU it lands on; potrf_diag needs a CU with 133 KB free and
        // sits upstream of the signal, so a wide poller deadlocks the chain until its spin bound expires
        // (observed at m = 16384 with 254 pollers).  Only launches that leave most CUs untouched may poll.
        s.crit_flag = fs && s.rem > NB && tb_wgs <= 64;
        if (s.crit_flag) s.poll_count = gemm_tiles(NB, NB, 32, 128, 0, 0);           // workgroups of the critical panel launch
        // Two-level blocking (dense handles): the steps come in groups of `gs` block columns.  A step updates only the
        // remaining columns of its group (a window of K = 128 tiles) and DEFERS the rest of its trailing update; the last
        // step of the group applies all of them at once with K = 128 gs -- the group's panels are adjacent block columns
        // of L, i.e. one k-contiguous operand -- so the trailing matrix, whose read-modify-write is what bounds a
        // K = 128 update (16 flop/byte), is streamed once per group instead of once per step.
        const bool inner = k + 1 < s.gend;                          // not the last column of its group: window only
        if (!inner && k > s.g0) s.kcols = k - s.g0 + 1;             // operands: block columns g0..k, rows >= k+1
        if (s.rem <= NB) continue;                                  // only the critical tile (k+1,k+1)
        int wgs;
        bool counter;
        if (inner) {
            // window: tiles (i, j), i >= k+2, k+1 <= j < gend:  B(i,j) -= L(i,k) L(j,k)^T as ONE rectangular GEMM.
            // Inside the group it also touches a few tiles above the diagonal (i < j), which nobody reads.
            s.window = std::min(s.gend - (k + 1), s.rem / NB);
            wgs = gemm_tiles(s.rem - NB, s.window * NB, 128, 128, 0, 0);
            counter = fs;
        } else {
            // the per-workgroup release (L2 write-back) of the counter protocol only pays in the latency-bound
            // regime; a throughput-bound update (thousands of tiles: 16k: 40 -> 50 ms) keeps the stream event
            wgs = gemm_tiles(s.rem, s.rem, 128, 128, 1, /*skip_first=*/1);
            counter = fs && wgs <= 1024;
        }
        s.bulk = counter ? CH_COUNTER : CH_EVENT;
        if (counter) s.bulk_count = wgs;
        ++(counter ? p.n_counter_steps : p.n_event_steps);
    }
    return p;
}

}  // namespace ipm
