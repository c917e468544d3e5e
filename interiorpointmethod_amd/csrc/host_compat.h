// host_compat.h -- host side of libipm_hip.so, unit 1b: which OPTIONS a handle may hold together, and why.  variant_legal
// (vector_ops.h) states which kernel classes exist; this is the layer above it.  One table of exclusion rows, one reader of the handle
// (feature_on), one refusal (compat_refuse) that every setter and entry point calls in place of a ladder of its own, and the three
// per-column rules (column_conflict).  Clearing a feature never consults the table.  The Python front ends hold the same rows
// (options.py); tests/test_compat_table_host.py compares the two through ipm_debug_compat.
// Single translation unit: included by ipm_api.hip behind host_handle.h, `static` functions only.
#pragma once

// THE place that maps a feature (include/ipm_hip.h: IPM_FEATURE_*) to handle fields.
static bool feature_on(const ipm_handle* h, int f) {
    switch (f) {
    case IPM_FEATURE_BOUNDS: return h->bnd;
    case IPM_FEATURE_QUADRATIC: return h->quad;
    case IPM_FEATURE_FREE: return h->free_set.on;
    case IPM_FEATURE_FREE_LP: return h->free_lp_set.on;
    case IPM_FEATURE_DETECT: return h->detect;
    case IPM_FEATURE_DETECT_QP: return h->detect_qp;
    case IPM_FEATURE_CORRECTORS: return h->mcc.k > 0;
    case IPM_FEATURE_REFINEMENT: return h->ref.k > 0;
    case IPM_FEATURE_DENSE_SPLIT: return !h->ds_cols.empty();
    case IPM_FEATURE_LOCKSTEP: return h->lockstep != 0;
    case IPM_FEATURE_LOCKSTEP_BOUNDS: return (h->opt.flags & IPM_FLAG_LOCKSTEP_BOUNDS) != 0;
    case IPM_FEATURE_SMALL_PATH: return h->small;
    case IPM_FEATURE_SMALL_QUADRATIC_FLAG: return (h->opt.flags & IPM_FLAG_SMALL_QUADRATIC) != 0;
    case IPM_FEATURE_SMALL_FREE_FLAG: return (h->opt.flags & IPM_FLAG_SMALL_FREE) != 0;
    default: return false;                                     // (IPM_FEATURE_MEHROTRA_START: an operation, never held)
    }
}
static int feature_count(const ipm_handle* h, int f) { return f == IPM_FEATURE_CORRECTORS ? h->mcc.k : f == IPM_FEATURE_REFINEMENT ? h->ref.k : 0; }   // the %d of a clause

// A row: a and b do not share a handle unless `lifted_by` (a feature or an option flag, -1: nothing) is on.  a_on: the "because" of the
// refusal when a is switched on beside b; b_on: when b is switched on beside a, where tests pin other words for that call order ("clear
// that set first" stands in one direction only) -- the pair, the rule and the lift are stated once.  b_on == nullptr: no entry point
// ever reports that order (b is fixed at ipm_create, or is the path ipm_set_A_csc chooses, which declines silently).
// one_way: switching b on beside a is NOT refused (the parent's behaviour, kept; each such row says what happens instead).
// A clause may hold one %d: the rounds set on the partner.  Rows are walked in table order, which is the order of every setter's former
// ladder: the first failure reported for any input is unchanged.
struct CompatRow { int a, b, lifted_by; bool one_way; const char *a_on, *b_on; };
#define NO_TWINS(what) "the handle was created with IPM_FLAG_LOCKSTEP (the " what " have no batched twins)"
#define SET_BEFORE_A "set them before A (ipm_set_A_csc then takes the multi-kernel path)"
static const CompatRow COMPAT_ROWS[] = {
    {IPM_FEATURE_QUADRATIC, IPM_FEATURE_FREE_LP, -1, false,
     "the handle holds LP free columns (ipm_set_free_lp_columns): they live on a handle without a quadratic term; clear that set first",
     "the handle holds a quadratic term (ipm_set_quadratic): LP free columns live on a handle without one (a free column with g > 0 is ipm_set_free_columns)"},
    {IPM_FEATURE_FREE, IPM_FEATURE_FREE_LP, -1, false,
     "the handle holds LP free columns (ipm_set_free_lp_columns): the two sets do not share a handle; clear that set first",
     "the handle holds free columns with curvature (ipm_set_free_columns): the two sets do not share a handle"},
    {IPM_FEATURE_QUADRATIC, IPM_FEATURE_LOCKSTEP, -1, false, NO_TWINS("Quad kernels"), nullptr},
    {IPM_FEATURE_FREE, IPM_FEATURE_LOCKSTEP, -1, false, NO_TWINS("Free kernels"), nullptr},
    {IPM_FEATURE_FREE_LP, IPM_FEATURE_LOCKSTEP, -1, false, NO_TWINS("free_lp kernels"), nullptr},
    {IPM_FEATURE_QUADRATIC, IPM_FEATURE_DETECT, IPM_FEATURE_DETECT_QP, false,
     "the handle was created with IPM_FLAG_DETECT_INFEASIBILITY (the dual ray of a QP also needs g o x = 0; the tests are not restated)", nullptr},
    {IPM_FEATURE_FREE, IPM_FEATURE_DETECT, IPM_FEATURE_DETECT_QP, false,
     "the handle was created with IPM_FLAG_DETECT_INFEASIBILITY (the tests are the LP's and are not restated)", nullptr},
    {IPM_FEATURE_FREE_LP, IPM_FEATURE_DETECT, -1, false,
     "the handle was created with IPM_FLAG_DETECT_INFEASIBILITY (the tests are not restated for LP free columns)", nullptr},
    {IPM_FEATURE_QUADRATIC, IPM_FEATURE_CORRECTORS, -1, false,
     "%d centrality correctors are set (their accept rule compares step pairs, a quadratic handle takes one step; ipm_set_centrality_correctors(h, 0))",
     "the handle holds a quadratic term (ipm_set_quadratic): it takes one step length, and the rounds' accept rule compares step pairs"},
    {IPM_FEATURE_FREE_LP, IPM_FEATURE_CORRECTORS, -1, false,
     "%d centrality correctors are set (their kernels are not restated for LP free columns; ipm_set_centrality_correctors(h, 0))",
     "the handle holds LP free columns (ipm_set_free_lp_columns): the rounds' kernels are not restated for them"},
    // the one-workgroup small path: ipm_set_A_csc switches it on, and DECLINES it (the multi-kernel path, no error) where a row excludes it
    {IPM_FEATURE_QUADRATIC, IPM_FEATURE_SMALL_PATH, IPM_FEATURE_SMALL_QUADRATIC_FLAG, false,
     "the handle runs the fused small-LP kernel, which has no quadratic term; set the term before A (ipm_set_A_csc then takes the multi-kernel path)", nullptr},
    {IPM_FEATURE_FREE, IPM_FEATURE_SMALL_PATH, IPM_FEATURE_SMALL_FREE_FLAG, false,
     "the handle runs the fused small kernel, which has no free columns; " SET_BEFORE_A, nullptr},
    {IPM_FEATURE_FREE_LP, IPM_FEATURE_SMALL_PATH, -1, false,
     "the handle runs the fused small kernel, which has no LP free columns; " SET_BEFORE_A, nullptr},
    // one-way: a handle that holds rounds still goes onto the small path (ipm_set_A_csc), and its solve entries refuse (rounds_check_path)
    {IPM_FEATURE_CORRECTORS, IPM_FEATURE_SMALL_PATH, -1, true,
     "the handle runs the fused small-LP kernel (one workgroup holds the whole loop; factor and solve cost the same there)", nullptr},
    {IPM_FEATURE_REFINEMENT, IPM_FEATURE_SMALL_PATH, -1, true,
     "the handle runs the fused small-LP kernel (one workgroup holds the whole loop; it has no rounds)", nullptr},
    {IPM_FEATURE_CORRECTORS, IPM_FEATURE_LOCKSTEP, -1, false, NO_TWINS("rounds"), nullptr},
    {IPM_FEATURE_REFINEMENT, IPM_FEATURE_LOCKSTEP, -1, false, NO_TWINS("rounds"), nullptr},
    {IPM_FEATURE_DENSE_SPLIT, IPM_FEATURE_LOCKSTEP, -1, false, "a lockstep handle has no split (its kernels have no batched twins)", nullptr},
    {IPM_FEATURE_DETECT_QP, IPM_FEATURE_LOCKSTEP, -1, false, "(the Quad and Free kernels have no batched twins)", nullptr},   // (two flags: ipm_create reports it)
    // one-way: ipm_set_bounds on a lockstep handle is accepted; the handle is refused where it JOINS a batch (ipm_solve_batch, and
    // ipm_batch_add in the batch's own words: ls_bounds_ok)
    {IPM_FEATURE_LOCKSTEP, IPM_FEATURE_BOUNDS, IPM_FEATURE_LOCKSTEP_BOUNDS, true, "the handle has upper bounds (ipm_set_bounds): no lockstep twin", nullptr},
    // one-way: the start is an operation, nothing is held afterwards
    {IPM_FEATURE_MEHROTRA_START, IPM_FEATURE_FREE, -1, true,
     "the handle has free columns (ipm_set_free_columns): the least-squares start is not restated for them; use ipm_init_state", nullptr},
};
#undef NO_TWINS
#undef SET_BEFORE_A

// the clause of row r when `f` is switched on beside the row's other feature (nullptr: the row does not refuse that order)
static const char* compat_clause(const CompatRow& r, int f, int* partner) {
    if (r.a == f) { *partner = r.b; return r.a_on; }
    if (r.b == f && !r.one_way) { *partner = r.a; return r.b_on ? r.b_on : r.a_on; }
    return nullptr;
}
// the table's answer for the ordered pair (switch a on, b held): the row, or nullptr
static const CompatRow* compat_row(int a, int b) {
    for (const CompatRow& r : COMPAT_ROWS) {
        int p;
        if (compat_clause(r, a, &p) && p == b) return &r;
    }
    return nullptr;
}
// THE reader: the clause of the first row, in table order, that refuses switching `f` on on this handle -- its partner on, its lift
// not -- or nullptr.  *partner_out receives the partner; only >= 0: that partner's row alone is asked.
static const char* compat_blocker(const ipm_handle* h, int f, int* partner_out = nullptr, int only = -1) {
    for (const CompatRow& r : COMPAT_ROWS) {
        int p;
        const char* clause = compat_clause(r, f, &p);
        if (!clause || (only >= 0 && p != only) || !feature_on(h, p) || (r.lifted_by >= 0 && feature_on(h, r.lifted_by))) continue;
        if (partner_out) *partner_out = p;
        return clause;
    }
    return nullptr;
}
// THE refusal: `who` (an entry point) is about to switch `f` on (only: as compat_blocker).  `member` >= 0: a batch entry names its member ("handle 3 has ..."
// for "the handle has ..."); to_handle = false: the message goes to the thread's record only, as the small batch's entries report.
static int compat_refuse(ipm_handle* h, const char* who, int f, int member = -1, bool to_handle = true, int only = -1) {
    int p;
    const char* clause = compat_blocker(h, f, &p, only);
    if (!clause) return IPM_OK;
    char why[400];
    snprintf(why, sizeof why, clause, feature_count(h, p));
    if (member < 0) return fail(h, IPM_ERR_INVALID_ARG, "%s: %s", who, why);
    static const char subject[] = "the handle ";
    const bool named = !strncmp(why, subject, sizeof subject - 1);
    return fail(to_handle ? h : nullptr, IPM_ERR_INVALID_ARG, named ? "%s: handle %d %s" : "%s: handle %d: %s", who, member, named ? why + sizeof subject - 1 : why);
}

// A requirement, not an exclusion: a free column needs its curvature, and a set given BEFORE the term is checked against it by
// ipm_set_quadratic -- if none ever came, the solve entries refuse (check_ready, ipm_solve_small_batch).  -> that set's first column, or -1.
static int free_without_term(const ipm_handle* h) { return h->free_set.on && !h->quad ? h->free_set.cols[0] : -1; }
static const char FREE_NEEDS_TERM[] = "is a free column (ipm_set_free_columns) without a quadratic term: a free column needs g > 0 (ipm_set_quadratic)";

// THE per-column rules: a free column (of either set) takes no finite bound, and a free column with curvature needs g_j > 0.  A setter
// asks for each column it touches, naming the feature it is setting (`what`: bounds / quadratic / free / free_lp) and, for the first
// two, the value v it gives the column; the rest of the column is read from the handle.
static int column_conflict(ipm_handle* h, const char* who, int what, int64_t j, double v = 0.0) {
    const long long c = (long long)j;
    if (what == IPM_FEATURE_BOUNDS) {                          // v: a finite bound
        if (h->free_set.has(j)) return fail(h, IPM_ERR_INVALID_ARG, "%s: u[%lld] = %g is finite, but column %lld is a free column (ipm_set_free_columns): it takes no bound", who, c, v, c);
        if (h->free_lp_set.has(j)) return fail(h, IPM_ERR_INVALID_ARG, "%s: u[%lld] = %g is finite, but column %lld is an LP free column (ipm_set_free_lp_columns): it takes no bound", who, c, v, c);
        return IPM_OK;
    }
    if (what == IPM_FEATURE_QUADRATIC) {                       // v: g_j (0 where no term is given); a free column keeps its curvature: 1 / g_j is its scaling
        if (h->free_set.has(j) && !(v > 0.0)) return fail(h, IPM_ERR_INVALID_ARG, "%s: g[%lld] = %g, but column %lld is a free column (ipm_set_free_columns) and needs g > 0; clear the free set first", who, c, v, c);
        return IPM_OK;
    }
    if (what == IPM_FEATURE_FREE && h->quad && !h->quad_pos[(size_t)j]) return fail(h, IPM_ERR_INVALID_ARG, "%s: column %lld has g = 0: a free column needs curvature (ipm_set_quadratic)", who, c);
    if (h->bnd && h->bnd_finite[(size_t)j]) return fail(h, IPM_ERR_INVALID_ARG, "%s: column %lld has a finite upper bound (ipm_set_bounds): a free column takes none", who, c);
    return IPM_OK;
}
