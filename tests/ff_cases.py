"""Shared by tests/test_ff_schedule.py (CPU) and tests/test_gpu_ff_schedule.py (GPU): the settings of the fused formation +
factorization's work-list generator (csrc/ff_schedule.h) that the tests sweep, and a restatement of its K-chunk cut formula."""
import math

# IPM_FF_MODEL perturbations: each moves the calibrated durations far enough to REORDER the list, none changes what an item
# computes (the cuts, batches and flags are not functions of the durations).  The CPU tests prove both of these claims.
MODELS = (
    "t_col=4,t_base=30",                        # cheap updates, dear slab adds
    "f_stage=9,f_over=25",                      # slow formation
    "potrf=150,cpanel=30,cupdate=30",           # slow pivot chain
    "handoff=12,gap=6,t_panel=60",              # slow hand-offs, dear panel solves
)

# one generator knob at a time (the environment variables ff_build_schedule reads itself)
KNOBS = (
    [("IPM_FF_BATCH", v) for v in ("1", "3", "8")]
    + [("IPM_FF_TAIL", v) for v in ("1", "4")]
    + [("IPM_FF_STAGGER", v) for v in ("0", "0.9")]
    + [("IPM_FF_Q_LAST", v) for v in ("8", "16")]
)


def pair_chunks(nblk, q, nstages, stagger=0.3, q_last=0, qmax=16):
    """{(i, c): [(s0, s1), ...]} for every formation tile pair (i even), re-evaluated the way ff_build_schedule cuts the K loop
    (same pair numbering, phase, rounding and IEEE double operations in the same order)."""
    out = {}
    npairs = 0
    for i in range(0, nblk, 2):
        for c in range(min(i + 1, nblk - 1) + 1):
            qq = q_last if (q_last > 0 and i + 2 >= nblk) else q
            qq = max(1, min(min(qq, max(qmax, q)), nstages))
            phi = math.fmod(npairs * 0.381966, 1.0)
            npairs += 1
            lens = [1.0 + stagger * (2.0 * math.fmod(k / qq + phi, 1.0) - 1.0) for k in range(qq)]
            tot = 0.0
            for v in lens:
                tot += v
            cut, acc = [0], 0.0
            for v in lens:
                acc += v
                cut.append(int(nstages * acc / tot + 0.5))
            cut[qq] = nstages
            out[(i, c)] = list(zip(cut[:-1], cut[1:]))
    return out
