"""Item costs of ONE fused launch from an item trace saved by tools/ff_trace.py (IPM_FF_TRACE_ITEMS=1): what FFModel's update
constants (csrc/ff_schedule.h: t_over, t_col, t_rmw, t_base) are calibrated on.  Usage:  python tools/ff_item_costs.py trace.npz
  * plain T items (no ADD_BASE, no PANEL, not INIT) by width: median work (inputs ready -> done), p10, p90; the fit
    work = fixed + per_column * columns through the medians of the 1- and 4-column items;
  * the base add per slab: ADD_BASE items without PANEL, by (width, slabs, INIT), median work minus the median of the plain
    items of the same width (width 0: minus the fitted fixed part), divided by the slabs; an INIT item reads no old tile;
  * drawn -> inputs ready of the T items (the polls of an item whose inputs are already there: the median);
  * worker work sums for F and T."""
import sys

import numpy as np

FF_F, FF_T = 0, 1
INIT, ADD_BASE, PANEL = 1, 2, 4


def pct(v):
    return np.median(v), np.percentile(v, 10), np.percentile(v, 90)


def main(path, out=sys.stdout):
    z = np.load(path)
    nit, items = int(z["nit"]), z["items"]
    it = z["trace"][:4 * nit].reshape(nit, 4).astype(np.float64)
    typ, ti, tc = items[:, 0], items[:, 1].astype(int), items[:, 2].astype(int)
    nblk = int(ti.max()) + 1
    F, T = typ == FF_F, typ == FF_T
    width = items[:, 5].astype(int) - items[:, 4].astype(int)
    flags = items[:, 6].astype(int)
    work = (it[:, 2] - it[:, 1]) / 100.0                  # 100 MHz clock -> microseconds
    wait = (it[:, 1] - it[:, 0]) / 100.0
    fdur = (it[:, 2] - it[:, 0]) / 100.0
    # slabs per tile: the live tiles of every formation chunk
    slabs = {}
    for n in np.nonzero(F)[0]:
        for r in (ti[n], ti[n] + 1):
            if tc[n] <= r < nblk:
                slabs[(r, tc[n])] = slabs.get((r, tc[n]), 0) + 1
    print("items %d (F %d, T %d), workers %d" % (nit, F.sum(), T.sum(), int(it[:, 3].max()) + 1), file=out)
    plain = T & ((flags & (INIT | ADD_BASE | PANEL)) == 0)
    med = {}
    for w in sorted(set(width[plain])):
        v = work[plain & (width == w)]
        med[w] = np.median(v)
        print("T plain, %d column(s): %4d items, work median %.2f us (p10 %.2f p90 %.2f, spread %.2f)" % ((w, v.size) + pct(v) + (np.percentile(v, 90) - np.percentile(v, 10),)), file=out)
    fixed = None
    if 1 in med and 4 in med:
        col = (med[4] - med[1]) / 3.0
        fixed = med[1] - col
        print("T plain fit through the 1- and 4-column medians: fixed %.2f us + %.2f us per column" % (fixed, col), file=out)
    base = T & ((flags & ADD_BASE) != 0) & ((flags & PANEL) == 0)
    qn = np.array([slabs.get((ti[n], tc[n]), 0) for n in range(nit)])
    per_slab = []
    for w in sorted(set(width[base])):
        ref = med.get(w, fixed if w == 0 else None)
        if ref is None:
            continue
        for q in sorted(set(qn[base & (width == w)])):
            for ini in (0, 1):
                sel = base & (width == w) & (qn == q) & (((flags & INIT) != 0) == bool(ini))
                if sel.sum() < 4 or q == 0:
                    continue
                v = (work[sel] - ref) / q
                per_slab.append((sel.sum(), np.median(v)))
                print("T ADD_BASE%s, %d column(s), %d slab(s): %4d items, (work - plain %.2f) / slabs median %.2f us (p10 %.2f p90 %.2f, spread %.2f)" % (
                    (" INIT" if ini else "     ", w, q, sel.sum(), ref) + pct(v) + (np.percentile(v, 90) - np.percentile(v, 10),)), file=out)
    if per_slab:
        print("base add per slab, item-weighted mean of the medians above: %.2f us" % (sum(c * m for c, m in per_slab) / sum(c for c, _ in per_slab)), file=out)
    print("T drawn -> inputs ready: median %.2f us (p10 %.2f p90 %.2f); sum %.0f us-CU" % (pct(wait[T]) + (wait[T].sum(),)), file=out)
    print("work sums: F %.0f us-CU, T %.0f us-CU (T wait %.0f); last item done at %.0f us" % (
        fdur[F].sum(), work[T].sum(), wait[T].sum(), (it[:, 2].max() - it[:, 0][it[:, 0] > 0].min()) / 100.0), file=out)


if __name__ == "__main__":
    main(sys.argv[1])
