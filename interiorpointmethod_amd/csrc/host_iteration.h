// host_iteration.h -- host side, unit 6: the launch sequence of one Mehrotra predictor-corrector iteration, the scalar read-back,
// the roll-back / recovery after a poll time-out, and the loops built on them (ipm_newton_direction, ipm_iterate, ipm_solve).
#pragma once
// The operations of a round feature (host_handle.h: Rounds), each stated once for the centrality correctors (h->mcc)
// and the iterative refinement (h->ref, 4-I).  With k = 0 nothing is enqueued anywhere, also on a handle that ran rounds before.
// The allocation, on first use, zeroed: products with A read the padding of the vectors in it, and the tallies start at zero.
template <class R> static int rounds_ensure(ipm_handle* h, R& r) {
    if (r.mem) return IPM_OK;
    const size_t n = r.kind->doubles(h);
    if (dev_malloc(h->device, h->stream, (void**)&r.mem, sizeof(double) * n) != hipSuccess)
        return fail(h, IPM_ERR_HIP, "%s: %lld doubles could not be allocated", r.kind->noun, (long long)n);
    HIP_TRY(h, hipMemsetAsync(r.mem, 0, sizeof(double) * n, h->stream));
    return IPM_OK;
}
template <class R> static bool rounds_on(const R& r) { return r.k > 0 && r.mem != nullptr; }
// start of a solve / of a sequence whose iteration count restarts (reset): the tallies restart with it.  With k > 0 the record is
// made here, in front of the roll-back snapshot; with k = 0 the host copy of the tallies is cleared on the host.
template <class R> static int rounds_start(ipm_handle* h, R& r, bool reset) {
    if (r.k <= 0) { if (reset) r.host = {}; return IPM_OK; }
    int rc = rounds_ensure(h, r);
    if (rc) return rc;
    if (reset) HIP_TRY(h, hipMemsetAsync(r.ctl(h), 0, sizeof r.host, h->stream));
    return IPM_OK;
}
// A handle that went onto the fused small path AFTER k > 0 was set (ipm_set_A_csc decides the path): its loop runs in one workgroup
// and has no rounds, so the solve entries refuse instead of dropping the option.
template <class R> static int rounds_check_path(ipm_handle* h, const R& r, const char* who) {
    if (h->small && r.k > 0)
        return fail(h, IPM_ERR_INVALID_ARG, "%s: %d %s are set but the handle runs the fused small-LP kernel, which has %s (%s(h, 0))", who, r.k, r.kind->noun, r.kind->none, r.kind->setter);
    return IPM_OK;
}
// the record -> its host copy, beside the scalar record (read_scalars); the record <-> its roll-back copy (enqueue_snapshot)
template <class R> static int rounds_read_back(ipm_handle* h, R& r) {
    if (rounds_on(r)) HIP_TRY(h, hipMemcpyAsync(&r.host, r.ctl(h), sizeof r.host, hipMemcpyDeviceToHost, h->stream));
    return IPM_OK;
}
template <class R> static int rounds_snapshot(ipm_handle* h, const R& r, int restore, hipStream_t st) {
    if (rounds_on(r)) HIP_TRY(h, hipMemcpyAsync(restore ? r.ctl(h) : r.ctl_copy(h), restore ? r.ctl_copy(h) : r.ctl(h), sizeof r.host, hipMemcpyDeviceToDevice, st));
    return IPM_OK;
}
// The setters' argument rules.  The range check reads nothing of the handle, so it comes first: both argument checks hold without a
// device, for any h.  k = 0 is accepted on every handle: it is the way out for a handle that went onto the small path after k > 0.
template <class R> static int rounds_set(ipm_handle* h, R ipm_handle::*which, const RoundsKind& kind, int32_t k) {
    if (k < 0 || k > kind.kmax) return fail(h, IPM_ERR_INVALID_ARG, "%s: k = %d outside 0 .. %d", kind.setter, (int)k, kind.kmax);
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "%s: NULL handle", kind.setter);
    if (k > 0) if (int rc_ = compat_refuse(h, kind.setter, kind.feature)) return rc_;
    (h->*which).k = k;
    return IPM_OK;
}

// One solve with the factored normal matrix, the one statement of it (predictor, corrector, a centrality-corrector round,
// ipm_normal_solve, the two solves of Mehrotra's start, refinement's own correction solve):  out = B~^-1 rhs with the handle's
// sweeps (rhs is consumed), then A^T out as partials into `atp` (null: no pass), then, for a `refine`d solve of a handle with
// ref.k > 0, the refinement rounds -- which need rhs kept in front of the sweeps and the A^T pass behind them.
// Hooks of the iteration: wait_last (enqueue_potrs), ev (two profiling events, around the sweeps) and stream_at.
// Streamed A^T dy (stream_at where stream_at_on): the backward sweep makes dy final one 1024-row group
// at a time, last group first, and the pass over A splits by row chunks without changing a bit (launch_gemv_t_rows), so the piece of
// every sweep event but the last runs on the residual stream while the sweep goes on: a gate on the handle's progress word (the
// bounded spin of every device-side wait; a time-out is rolled back like any other and poll_fallback drops the streaming for good),
// then the piece.  The main stream runs the last event's piece itself and joins the residual stream with one event wait -- that
// event is recorded behind the last streamed piece, which has normally ended by then.
// h->atp: the corrector's pieces overwrite the predictor's partials, which mu_aff / corrector_rhs / the predictor's direction
// kernel read -- all of them IN FRONT of the corrector's sweep on the main stream, and a piece runs only behind the gate that a
// kernel of that sweep opens.  The next iteration's A^T y (residual stream) is enqueued behind these pieces on the same in-order
// stream, and behind this iteration's last reader through the event it waits for (ev_mid / ev_fork, recorded on the main stream).
struct SolveHooks { hipEvent_t wait_last = nullptr; hipEvent_t* ev = nullptr; bool stream_at = false; };
static int refine_keep(ipm_handle* h, const double* t);
static int enqueue_refine(ipm_handle* h, double* dy);
static int enqueue_normal_solve(ipm_handle* h, double* rhs, double* out, double* atp, bool refine, const SolveHooks& hooks = {}) {
    int rc;
    if (((refine && h->ref.k > 0) || hooks.stream_at) && atp != h->atp)             // (both read and write the handle's own partials)
        return fail(h, IPM_ERR_INVALID_ARG, "enqueue_normal_solve: a refined or streamed solve takes h->atp");
    if (hooks.ev) HIP_TRY(h, hipEventRecord(hooks.ev[0], h->stream));
    if (refine && (rc = refine_keep(h, rhs))) return rc;
    std::vector<AtPiece> pieces;
    if (hooks.stream_at && stream_at_on(h)) pieces = at_piece_schedule(h->mp, h->gsz, h->nblk, h->rc_chunks, h->rows_per_chunk);
    if (pieces.empty()) {
        if ((rc = enqueue_potrs(h, rhs, out, hooks.wait_last))) return rc;
        if (hooks.ev) HIP_TRY(h, hipEventRecord(hooks.ev[1], h->stream));
        if (atp) launch_gemv_t(h, out, nullptr, atp);
    } else {
        bool streamed = false;
        SweepHook hook;
        hook.word = at_progress_word(h); hook.base = h->at_epoch;
        h->at_epoch += (unsigned)pieces.size();
        hook.released = [&](int e) {                             // (the kernel that signals event e is enqueued: the gate goes behind it)
            const AtPiece& p = pieces[(size_t)e];
            if (p.chunk1 <= p.chunk0) return;
            hipLaunchKernelGGL(ff_gate_kernel, dim3(1), dim3(64), 0, h->stream3, hook.word, hook.base + (unsigned)e + 1u, timeout_word(h), &h->sc->done);
            launch_gemv_t_rows(h, out, p.chunk0, p.chunk1, h->stream3);
            streamed = true;
        };
        if ((rc = enqueue_potrs(h, rhs, out, hooks.wait_last, &hook))) return rc;
        if (hooks.ev) HIP_TRY(h, hipEventRecord(hooks.ev[1], h->stream));
        launch_gemv_t_rows(h, out, pieces.back().chunk0, pieces.back().chunk1, h->stream);
        if (streamed) {
            HIP_TRY(h, hipEventRecord(h->ev_at, h->stream3));
            HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_at, 0));
        }
    }
    return refine ? enqueue_refine(h, out) : IPM_OK;              // (streamed pieces: behind the join)
}

// Iterative refinement of a solve (iteration_rules.h: refine_decide; refine_ops.h), the two halves that bracket it
// inside enqueue_normal_solve: refine_keep copies the right-hand side in front of the sweeps, which consume it, and enqueue_refine
// goes behind the A^T dy pass: ref.k rounds of residual -> decide -> delta = B~^-1 r, A^T delta (a solve of its own, unrefined,
// into the feature's buffers) -> apply.  That solve tests RefCtl::rdone, which the decide kernel of the round wrote: once the
// rounds of a solve have ended, what is left of them are launches that return at entry, and the host never looks.  The residual is
// taken with the handle's current D^2 vector h->d (theta on a bounded handle).  All launches are on the main stream and untwinned
// (ipm_set_refinement refuses a lockstep handle; a program recorded with rounds pending would be cut).
// h->atp: the apply kernel rewrites the partials in place, in front of their readers on this stream (direction_kernel and, for the
// predictor, mu_aff / corrector_rhs); the next writer is ordered behind them as said below for the centrality correctors.
static int refine_keep(ipm_handle* h, const double* t) {
    if (h->ref.k <= 0) return IPM_OK;
    int rc = rounds_ensure(h, h->ref);
    if (rc) return rc;
    launch_untwinned(h, refine_keep_kernel, dim3((unsigned)((h->mp + 255) / 256)), dim3(256), nullptr, t, ref_views(h).t, (int)h->mp, solve_done(h));
    return IPM_OK;
}
static int enqueue_refine(ipm_handle* h, double* dy) {               // dy: the result of the solve, whose A^T dy partials are in h->atp
    if (h->ref.k <= 0) return IPM_OK;
    int rc;
    const RefViews v = ref_views(h);
    const int* outer = solve_done(h);                               // the word of the solve (Scalars::done, or a corrector round's)
    const unsigned gres = (unsigned)(h->mp / REF_ROWS);
    const unsigned gapp = (unsigned)std::min<int64_t>(((int64_t)ref_na(h) + VBLK - 1) / VBLK, 1024);
    for (int j = 0; j < h->ref.k; ++j) {
        const int first = j == 0;
        if (h->sparse) launch_untwinned(h, refine_residual_csr_kernel, dim3(gres), dim3(256), nullptr, sparse_view(h), (int)h->mp, (int)h->np, (const double*)h->d,
                                        (const double*)h->atp, h->rc_chunks, (const double*)v.t, v.r, v.part, outer, (const RefCtl*)v.ctl, first);
        else launch_untwinned(h, refine_residual_dense_kernel, dim3(gres), dim3(256), nullptr, (const double*)h->A, h->np, (int)h->m, (int)h->mp, (int)h->n, (int)h->np,
                              (const double*)h->d, (const double*)h->atp, h->rc_chunks, (const double*)v.t, v.r, v.part, outer, (const RefCtl*)v.ctl, first);
        launch_untwinned(h, refine_decide_kernel, dim3(1), dim3(VBLK), nullptr, (const double*)v.part, (int)gres, v.ctl, outer, first);
        {
            SolveWord word(h, &v.ctl->rdone);
            if ((rc = enqueue_normal_solve(h, v.r, v.delta, v.atd, /*refine=*/false))) return rc;
        }
        launch_untwinned(h, refine_apply_kernel, dim3(gapp), dim3(VBLK), nullptr, (const RefCtl*)v.ctl, (int)h->m, (int64_t)ref_na(h), (const double*)v.delta,
                         (const double*)v.atd, dy, h->atp, v.dy_keep, v.atp_keep);
    }
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

// the tail the predictor (corr = 0) and the corrector (corr = 1) share: dy = B^{-1} t1, A^T dy, then the x and s parts of the direction
static int enqueue_solve_direction(ipm_handle* h, hipEvent_t* ev, double* dy, int corr, hipEvent_t wait_last = nullptr) {
    int rc = enqueue_normal_solve(h, h->t1, dy, h->atp, /*refine=*/true, {wait_last, ev, /*stream_at=*/true});
    if (rc) return rc;
    launch_direction(h, corr);
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}
static int enqueue_predictor(ipm_handle* h, hipEvent_t* ev, bool have_rhs = false, hipEvent_t wait_last = nullptr) {
    if (!have_rhs) launch_gemv_n(h, h->v, -1.0, -1.0, h->rb, h->t1);   // rhs = -r_b - A (d*t)
    return enqueue_solve_direction(h, ev, h->dya, 0, wait_last);
}
static int enqueue_corrector(ipm_handle* h, hipEvent_t* ev) {
    launch_mu_aff(h);
    launch_corrector_rhs(h);
    launch_gemv_n(h, h->v, -1.0, -1.0, h->rb, h->t1);
    return enqueue_solve_direction(h, ev, h->dy, 1);
}

// Centrality correctors: up to mcc.k rounds between the corrector and the update, each the corrector's pipeline
// again with this iteration's factor -- target / right-hand side, rhs = -r_b - A v_g, dy_g = B^{-1} rhs, A^T dy_g, the candidate
// direction, the accept decision.  The products with A and the substitutions test MccCtl::rdone (SolveWord), which the round's
// target kernel sets: after a rejected round the later rounds of the iteration are launches that return at entry.  t1 / t2 are
// free here (the corrector's solve consumed them) and the candidate vectors are mcc.mem.
// A^T dy_g is the UNSTREAMED pass on the main stream (streaming it behind the sweep is left out): it overwrites h->atp, whose last
// reader of the Mehrotra corrector (direction_kernel) lies in front of it on this stream.  The next writer of h->atp is the next
// iteration's A^T y on the residual stream; it waits for ev_mid (enqueue_residual_stream) or, on the fused path, ev_fork
// (enqueue_form_factor), both recorded on the MAIN stream inside that iteration's factorization -- behind launch_update and so
// behind every round's mcc_direction_kernel, the last reader of h->atp, in stream order.
static int enqueue_corrector_rounds(ipm_handle* h) {
    if (h->mcc.k <= 0) return IPM_OK;
    int rc = rounds_ensure(h, h->mcc);
    if (rc) return rc;
    const VecArgs c = mcc_vec_args(h);
    for (int r = 0; r < h->mcc.k; ++r) {
        launch_mcc_target(h, r == 0);
        {
            SolveWord word(h, &h->mcc.ctl(h)->rdone);
            launch_gemv_n(h, c.v, -1.0, -1.0, h->rb, h->t1);
            if ((rc = enqueue_normal_solve(h, h->t1, c.dy, h->atp, /*refine=*/true))) return rc;
        }
        launch_mcc_direction(h);
        launch_mcc_accept(h);
    }
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

// events per profiled iteration: 0 start, 1 before form, 2 after form, 3 after factor,
// 4/5 around predictor solve, 6/7 around corrector solve, 8 end
static const int EV_PER_IT = 9;

static int enqueue_iteration(ipm_handle* h, hipEvent_t* ev) {
    int rc;
    if ((rc = check_class(h, "enqueue_iteration"))) return rc;
    const bool all = ev && h->profiling >= 2;            // each event record costs the stream ~6 us: level 1 keeps two
    if (overlap_residuals(h)) {
        // d = x/s -> formation -> factorization, with the residuals, the stop test and the predictor rhs on the residual
        // stream under the chain-bound tail of the factorization
        launch_scaling(h);
        const bool fused = ff_use(h);                        // evaluated ONCE per iteration (the live-handle count can change under it)
        if (ev && !fused) HIP_TRY(h, hipEventRecord(ev[1], h->stream));
        // the stop test of THIS iterate runs on the residual stream while the factorization is in flight: formation and
        // factorization test the latch scaling_kernel took (Scalars::done_f), so they either run whole or not at all and
        // after a converged solve B / invD hold the complete factor of the final iterate (ipm_get_factor, pivots_fixed)
        struct Latch { ipm_handle* h; ~Latch() { h->fdone = nullptr; } } latch{h};
        h->fdone = &h->sc->done_f;
        h->ff_last = false;
        if (!fused) {
            if ((rc = enqueue_form(h, h->d))) return rc;
            if (ev) HIP_TRY(h, hipEventRecord(ev[2], h->stream));
        }
        // start late in the chain-bound tail: the three passes need ~0.2 ms, six steps of the chain.  Measured at 32 blocks
        // (it/s for a start at step 0 / 4 / 12 / 20 / 26 / 30): 199.5 / 199.6 / 200.6 / 201.0 / 203.1 / 200.5
        const int rstep = h->nblk * 13 / 16;
        const int nG = h->grouped_trsv ? h->nblk / h->gsz : 0;
        const int gstep = (nG >= 2 && (nG - 1) * h->gsz - 1 < rstep) ? (nG - 1) * h->gsz - 1 : -1;
        if (fused) { if ((rc = enqueue_form_factor(h, ev, rstep, gstep))) return rc; }
        else if ((rc = enqueue_factor(h, rstep, gstep))) return rc;
        // the explicit inverses of the diagonal groups are part of the factor (ipm_normal_solve with reuse_factor substitutes with
        // both): they test the latch as well, and so does the gate in front of them -- with `done` the last group's inverses of the
        // iteration whose stop test fired stayed those of the iterate before, under the factor of the final one
        if (gstep >= 0) {
            // the last group's inverse (nine dependent launches, ~80 us) goes to the residual stream as well: the forward
            // sweep of the predictor over the earlier groups runs beside it and only its last step waits
            if (h->ff_last && h->ff_potrfdone) {
                // fused launch: the residual stream does not wait for an EVENT behind the launch (in the kernel trace both streams
                // then resumed 45 us after the launch's last wave: two streams waiting for each other's events) but for the chain's
                // last hand-off word, like the gate of the earlier groups: behind it the whole factor is released at agent scope
                // (every worker's writes through the tile counters the chain acquired), and every kernel of a stream starts with an
                // acquire.  The last group's inverse now starts 2 us after the launch ends, the main stream's sweep 11 us
                // (profiles/r04_dense_iteration_timeline*.txt): 261.3 -> 262.4 it/s.
                hipLaunchKernelGGL(ff_gate_kernel, dim3(1), dim3(64), 0, h->stream3, h->ff_potrfdone + (h->nblk - 1), 1u, timeout_word(h), factor_done(h));
            } else {
                HIP_TRY(h, hipEventRecord(h->ev_grp, h->stream));
                HIP_TRY(h, hipStreamWaitEvent(h->stream3, h->ev_grp, 0));
            }
            if ((rc = enqueue_group_inverses(h, nG - 1, nG, h->stream3))) return rc;
            h->fdone = nullptr;
            HIP_TRY(h, hipEventRecord(h->ev_last, h->stream3));
            HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_res, 0));
            if ((rc = enqueue_predictor(h, nullptr, /*have_rhs=*/true, h->ev_last))) return rc;
        } else {
            if ((rc = enqueue_group_inverses(h, 0, nG, nullptr))) return rc;
            h->fdone = nullptr;
            HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_res, 0));
            if ((rc = enqueue_predictor(h, nullptr, /*have_rhs=*/true))) return rc;
        }
        if ((rc = enqueue_corrector(h, nullptr))) return rc;
        if ((rc = enqueue_corrector_rounds(h))) return rc;
        launch_update(h);
        HIP_TRY(h, hipGetLastError());
        return IPM_OK;
    }
    if (all) HIP_TRY(h, hipEventRecord(ev[0], h->stream));
    if ((rc = enqueue_residuals(h))) return rc;
    h->ff_last = false;
    bool have_rhs = false;
    if (h->profiling < 2 && ff_use(h)) {
        // (handles below 16 blocks have no residual stream: the fused launch is used here only when IPM_FUSED_FACTOR=force
        //  lowers the block limit -- the tests' way to run the fused kernels at small sizes)
        if ((rc = enqueue_form_factor(h, ev, -1, -1))) return rc;
    } else {
        if (ev) HIP_TRY(h, hipEventRecord(ev[1], h->stream));
        if ((rc = enqueue_form(h, h->d))) return rc;
        if (ev) HIP_TRY(h, hipEventRecord(ev[2], h->stream));
        if (sp_on(h) && h->sp_fuse_fwd) {
            // sparse factor: the predictor's right-hand side does not depend on the factor -- form it first and let its forward
            // substitution ride on the factorization (four walks of the elimination tree per iteration instead of five)
            launch_gemv_n(h, h->v, -1.0, -1.0, h->rb, h->t1);   // rhs = -r_b - A (d*t)
            have_rhs = true;
            if ((rc = enqueue_factor(h, -1, -1, h->t1))) return rc;
        } else if ((rc = enqueue_factor(h))) return rc;
    }
    if ((rc = enqueue_group_inverses(h))) return rc;
    if (all) HIP_TRY(h, hipEventRecord(ev[3], h->stream));
    if ((rc = enqueue_predictor(h, all ? ev + 4 : nullptr, have_rhs))) return rc;
    if ((rc = enqueue_corrector(h, all ? ev + 6 : nullptr))) return rc;
    if ((rc = enqueue_corrector_rounds(h))) return rc;         // (profiling: their time is part of phase 3, "other")
    launch_update(h);
    HIP_TRY(h, hipGetLastError());
    if (all) HIP_TRY(h, hipEventRecord(ev[8], h->stream));
    return IPM_OK;
}

// Host copy of the scalar record (one sync).  *timed_out (optional) receives the poll time-out word of the
// device-side hand-offs and the word is cleared; without it a time-out is an error.
static int read_scalars(ipm_handle* h, bool* timed_out = nullptr) {
    unsigned tmo = 0;
    unsigned* word = timeout_word(h);
    HIP_TRY(h, hipMemcpyAsync(h->h_sc, h->sc, sizeof(Scalars), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&tmo, word, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    int rc;
    if ((rc = rounds_read_back(h, h->mcc)) || (rc = rounds_read_back(h, h->ref))) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (tmo) {
        if (h->stream2) HIP_TRY(h, hipStreamSynchronize(h->stream2));               // the bulk stream may still be draining
        if (h->ff_built && h->ff_last && getenv("IPM_FF_DEBUG")) ff_dump_handoffs(h);
        HIP_TRY(h, hipMemsetAsync(word, 0, sizeof(unsigned), h->stream));
        if (!timed_out) return fail(h, IPM_ERR_HIP, "a device-side hand-off poll timed out (persistent solve)");
    }
    if (timed_out) *timed_out = tmo != 0;
    return IPM_OK;
}

// A poll time-out means a consumer gave up waiting and computed on stale tiles: the results of the call are
// garbage but nothing hung.  Policy: never surface it -- switch this handle to stream events for good, undo the
// call's effect on the iterate (callers restore their snapshot) and run it again.
static void poll_fallback(ipm_handle* h) {
    if (h->spf) h->sp_serial = true;          // sparse factor: one workgroup per launch from now on (it never waits)
    h->stream_at = 0;                         // A^T dy goes back behind the sweeps (its gates poll the device too)
    if (h->ff_last) h->ff_enabled = 0;        // the fused launch timed out: serial formation + factorization from now on, look-ahead kept
    else h->flag_sync = 0;
    ++h->timeouts_recovered;
}

// (x, y, s, Scalars) <-> roll-back buffer, one launch
__global__ __launch_bounds__(256) void snapshot_kernel(double* x, double* y, double* s, Scalars* sc, double* snap, int np,
                                                       int mp, int restore) {
    const int gid = blockIdx.x * 256 + threadIdx.x, gsz = gridDim.x * 256;
    double *sx = snap, *ss = snap + np, *sy = snap + 2 * (size_t)np;
    Scalars* ssc = (Scalars*)(snap + 2 * (size_t)np + mp);
    if (restore) {
        for (int j = gid; j < np; j += gsz) { x[j] = sx[j]; s[j] = ss[j]; }
        for (int i = gid; i < mp; i += gsz) y[i] = sy[i];
        if (gid == 0) *sc = *ssc;
    } else {
        for (int j = gid; j < np; j += gsz) { sx[j] = x[j]; ss[j] = s[j]; }
        for (int i = gid; i < mp; i += gsz) sy[i] = y[i];
        if (gid == 0) *ssc = *sc;
    }
}
__global__ __launch_bounds__(256) void snapshot_bounds_kernel(double* w, double* z, double* sw, double* sz, int np, int restore) {
    const int gid = blockIdx.x * 256 + threadIdx.x, gsz = gridDim.x * 256;
    for (int j = gid; j < np; j += gsz) {
        if (restore) { w[j] = sw[j]; z[j] = sz[j]; }
        else { sw[j] = w[j]; sz[j] = z[j]; }
    }
}
static int enqueue_snapshot(ipm_handle* h, int restore, hipStream_t st = nullptr) {
    const int64_t mx = h->np > h->mp ? h->np : h->mp;
    const unsigned grid = (unsigned)std::min<int64_t>((mx + 255) / 256, 256);
    hipLaunchKernelGGL(snapshot_kernel, dim3(grid), dim3(256), 0, st ? st : h->stream, h->x, h->y, h->s, h->sc, h->snap, (int)h->np,
                       (int)h->mp, restore);
    if (h->bnd) {                                              // (w, z) <-> their roll-back copies behind the bound vectors
        const BndArgs b = bnd_args(h);
        double* sw = h->bnd_mem + 8 * (size_t)h->np;
        hipLaunchKernelGGL(snapshot_bounds_kernel, dim3(grid), dim3(256), 0, st ? st : h->stream, b.w, b.z, sw, sw + h->np, (int)h->np, restore);
    }
    int rc;                                                    // the records of the rounds (their tallies) <-> the copies behind them
    if ((rc = rounds_snapshot(h, h->mcc, restore, st ? st : h->stream)) || (rc = rounds_snapshot(h, h->ref, restore, st ? st : h->stream))) return rc;
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}
// can the next factorization time out at all?  (the conservative superset of polls_device: see wants_polling)
static bool may_poll(const ipm_handle* h) { return (h->spf && !h->sp_serial && !sp_level(h)) || wants_polling(h); }

static void fill_stats(ipm_handle* h, ipm_stats* st, double ms) {
    if (!st) return;
    const Scalars& s = *h->h_sc;
    memset(st, 0, sizeof *st);
    st->status = s.status; st->iterations = s.k; st->pivots_fixed = s.fixed; st->auto_regularized = h->auto_reg;
    st->objective_last_finite = s.obj_last_finite;
    st->objective = s.obj; st->rp_norm = s.rb_norm; st->rd_norm = s.rc_norm; st->gap = s.gap;
    st->b_norm = s.b_norm; st->c_norm = s.c_norm; st->mu = s.mu; st->mu_aff = s.mu_aff; st->sigma = s.sigma;
    st->alpha_aff_p = s.alpha_aff_p; st->alpha_aff_d = s.alpha_aff_d; st->alpha_p = s.alpha_p; st->alpha_d = s.alpha_d;
    st->solve_ms = ms;
}

static int check_ready(ipm_handle* h, const char* who) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (!h->haveA || !h->haveBC || !h->haveState) return fail(h, IPM_ERR_STATE, "%s: A, (b,c) and a state must be set first", who);
    if (const int c = free_without_term(h); c >= 0) return fail(h, IPM_ERR_INVALID_ARG, "%s: column %d %s", who, c, FREE_NEEDS_TERM);
    return IPM_OK;
}

// ------------------------------------------------------------------------------- seams
extern "C" int ipm_newton_direction(ipm_handle* h, int corrector, double* dx, double* dy, double* ds, ipm_stats* stats) {
    int rc = check_ready(h, "ipm_newton_direction");
    if (rc) return rc;
    if ((rc = rounds_check_path(h, h->ref, "ipm_newton_direction"))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (!corrector) {
        for (int attempt = 0;; ++attempt) {                 // second pass only after a recovered poll time-out
            hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, 1e-8, 1e-8, 1e-8, h->opt.eta, 1 << 30, 1, 0);
            if ((rc = rounds_start(h, h->ref, true))) return rc;         // the tallies describe this call's solve
            if ((rc = enqueue_residuals(h))) return rc;
            if ((rc = enqueue_form(h, h->d))) return rc;
            if ((rc = enqueue_factor(h))) return rc;
            if ((rc = enqueue_group_inverses(h))) return rc;
            if ((rc = enqueue_predictor(h, nullptr))) return rc;
            launch_mu_aff(h);                                   // alpha_aff for stats
            bool tmo = false;
            if ((rc = read_scalars(h, &tmo))) return rc;
            if (!tmo) break;
            if (attempt) return fail(h, IPM_ERR_HIP, "hand-off time-out persists with stream events");
            poll_fallback(h);
        }
        h->predictor_valid = true;
        if (dx) HIP_TRY(h, hipMemcpyAsync(dx, h->dxa, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
        if (dy) HIP_TRY(h, hipMemcpyAsync(dy, h->dya, sizeof(double) * h->m, hipMemcpyDeviceToHost, h->stream));
        if (ds) HIP_TRY(h, hipMemcpyAsync(ds, h->dsa, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    } else {
        if (!h->predictor_valid) return fail(h, IPM_ERR_STATE, "corrector requested without a predictor at this state");
        if ((rc = rounds_start(h, h->ref, true))) return rc;
        if ((rc = enqueue_corrector(h, nullptr))) return rc;
        // alpha_p/alpha_d for stats without moving the iterate: recompute in a 1-thread kernel? they are
        // written by update_kernel only; expose the raw ratio minima through sigma/mu_aff and leave alpha to
        // ipm_iterate.  (The step lengths are checked end-to-end by the iterate tests.)
        if (dx) HIP_TRY(h, hipMemcpyAsync(dx, h->dx, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
        if (dy) HIP_TRY(h, hipMemcpyAsync(dy, h->dy, sizeof(double) * h->m, hipMemcpyDeviceToHost, h->stream));
        if (ds) HIP_TRY(h, hipMemcpyAsync(ds, h->ds, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    }
    if (corrector && (rc = read_scalars(h))) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    eq_out(h, dx, h->eq_c, false); eq_out(h, dy, h->eq_r, false); eq_out(h, ds, h->eq_c, true);      // scaled handle: C dx', R dy', ds' / C
    fill_stats(h, stats, 0.0);
    return IPM_OK;
}

// ------------------------------------------------------------------------------- centrality correctors
extern "C" int ipm_set_centrality_correctors(ipm_handle* h, int32_t k) {
    return rounds_set(h, &ipm_handle::mcc, MCC_KIND, k);
}
extern "C" int ipm_get_corrector_info(ipm_handle* h, int64_t out[4]) {
    if (!h || !out) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_corrector_info: bad arguments");
    const MccCtl& c = h->mcc.host;                              // the host copy the last ipm_solve / ipm_iterate read back
    out[0] = h->mcc.k; out[1] = c.run; out[2] = c.acc; out[3] = c.iters;
    return IPM_OK;
}

// ------------------------------------------------------------------------------- iterative refinement
extern "C" int ipm_set_refinement(ipm_handle* h, int32_t k) {
    if (h && h->ds_on && k >= 0 && k < DS_MIN_REFINE) k = DS_MIN_REFINE;      // a dense-column split keeps its own rounds
    return rounds_set(h, &ipm_handle::ref, REF_KIND, k);
}
extern "C" int ipm_debug_get_refine_vector(ipm_handle* h, int32_t which, double* out, int64_t capacity, int64_t* count) {
    if (!h || !count || which < 0 || which > 4) return fail(h, IPM_ERR_INVALID_ARG, "ipm_debug_get_refine_vector: bad arguments");
    *count = h->mp;
    if (!out || capacity < h->mp) return IPM_OK;
    if (which < 3 && !h->ref.mem) return fail(h, IPM_ERR_STATE, "ipm_debug_get_refine_vector: the handle never ran a refinement round");
    const RefViews v = h->ref.mem ? ref_views(h) : RefViews{};
    const double* src = which == 0 ? v.t : which == 1 ? v.r : which == 2 ? v.delta : which == 3 ? h->dy : h->dya;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(out, src, sizeof(double) * h->mp, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return IPM_OK;
}
extern "C" int ipm_get_refinement_info(ipm_handle* h, double out[8]) {
    if (!h || !out) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_refinement_info: bad arguments");
    const RefCtl& c = h->ref.host;                              // the host copy the last call that read the scalar record took
    out[0] = h->ref.k; out[1] = (double)c.solves; out[2] = (double)c.applied; out[3] = (double)c.half; out[4] = (double)c.reverts;
    out[5] = c.first_rel; out[6] = c.last_rel; out[7] = c.max_rel;
    return IPM_OK;
}

// arguments of the fused small-LP kernels for this handle (small_lp.h): the single-LP launch and the items of ipm_solve_small_batch
static SmallLP small_args(ipm_handle* h, int max_steps, int auto_reg) {
    SmallLP a;
    a.A = sparse_view(h); a.m = (int)h->m; a.n = (int)h->n; a.nt = (int)((h->m + 15) / 16);
    a.bptr = h->sm_bptr; a.bi = h->sm_bi; a.bk = h->sm_bk; a.bcol = h->sm_bcol; a.bcoef = h->sm_bcoef; a.nb = h->sm_nb;
    a.x = h->x; a.y = h->y; a.s = h->s; a.b = h->b; a.c = h->c;
    a.rc = h->rc; a.d = h->d; a.v = h->v; a.q = h->q; a.dxa = h->dxa; a.dsa = h->dsa; a.dx = h->dx; a.ds = h->ds;
    a.sc = h->sc; a.hist = h->hist;
    a.eps = h->opt.pivot_guard_eps; a.big = h->opt.pivot_guard_big; a.shift_rel = h->shift_rel;
    a.max_steps = max_steps; a.auto_reg = auto_reg;
    return a;
}

// The SMALL_* id of the handle's class: the row of the variant table (small_lp.h: SMALL_ROWS) whose switches are the handle's.
// (A quadratic term meets detect only with IPM_FLAG_DETECT_QUADRATIC, and free columns never meet a handle without a term:
//  check_ready / the batch's own check refuse that, so every handle that gets here has a row.)
static int small_variant(const ipm_handle* h) { return small_row_of(SMALL_ROWS, variant_bits(step_variant(h))); }
static SmallItem small_item(ipm_handle* h, int index, int max_steps, int auto_reg) {
    SmallItem it;
    memset(&it, 0, sizeof it);
    it.lp = small_args(h, max_steps, auto_reg);
    if (h->bnd) it.bd = bnd_args(h);
    it.dt = det_args(h);
    it.g = h->quad ? h->quad_g : nullptr;
    if (h->free_set.on) it.fr = free_args(h);
    it.eta = h->opt.eta;
    it.variant = small_variant(h);
    it.index = index;
    return it;
}
// A row of a variant table of the fused small-LP path (small_lp.h: SMALL_ROWS by SMALL_* id, SMALL_START_ROWS by bounded): `one`
// (a host item) launches the row's single-LP kernel on it, its arguments bound by type; otherwise the row's batch kernel runs
// `grid` workgroups on the device table d_items.
static void launch_small(const SmallRow& row, hipStream_t S, const SmallItem* one, const SmallItem* d_items, unsigned grid) {
    if (one) row.one(S, *one);
    else hipLaunchKernelGGL(row.batch, dim3(grid), dim3(PD_THREADS), 0, S, d_items);
}

// whole loop of a small sparse LP in one launch of one workgroup (small_lp.h)
static int enqueue_small(ipm_handle* h, int max_steps, int auto_reg) {
    if (int rc_ = check_class(h, "enqueue_small")) return rc_;
    const SmallItem it = small_item(h, 0, max_steps, auto_reg);
    launch_small(SMALL_ROWS[it.variant], h->stream, &it, nullptr, 1);
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

// Mehrotra's starting point of a multi-kernel handle, enqueued on the handle's stream (ipm_init_state_mehrotra):
// A A^T formed with d = 1, factored with the handle's guard and shift and the group inverses built as ipm_normal_solve(h, NULL, ...)
// does, then  u = (A A^T)^-1 b, x = A^T u  and  y = (A A^T)^-1 (A c), s = c - A^T y  from the device copies of b and c, then the
// shifts and the balance (vector_ops.h, start_*).  The guarded-pivot count of the factorization stays in sc->fixed.  Never part of a
// recorded lockstep program (the handle joins its batch afterwards).
static int enqueue_mehrotra_start(ipm_handle* h) {
    int rc;
    const unsigned gn = (unsigned)((h->n + 255) / 256);
    hipLaunchKernelGGL(fill_kernel, dim3(gn), dim3(256), 0, h->stream, h->d, (int)h->n, 1.0);
    if ((rc = enqueue_form(h, h->d))) return rc;
    if ((rc = enqueue_factor(h))) return rc;
    if ((rc = enqueue_group_inverses(h))) return rc;
    // x = A^T (A A^T)^-1 b   (the padding rows of b are zero, and stay zero through the solve)
    HIP_TRY(h, hipMemcpyAsync(h->t1, h->b, sizeof(double) * h->mp, hipMemcpyDeviceToDevice, h->stream));
    if ((rc = enqueue_normal_solve(h, h->t1, h->dy, h->atp, /*refine=*/false))) return rc;
    launch_step(STEP_START_PRIMAL, h);
    // y = (A A^T)^-1 (A c), s = c - A^T y
    launch_gemv_n(h, h->c, 1.0, 0.0, nullptr, h->t1);
    if ((rc = enqueue_normal_solve(h, h->t1, h->dy, h->atp, /*refine=*/false))) return rc;
    for (const StepTable* t : {&STEP_START_DUAL, &STEP_START_SHIFT, &STEP_START_PRIMAL_CORRECT, &STEP_START_DUAL_CORRECT}) launch_step(*t, h);
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

// what every entry that sets a new iterate leaves in the handle (ipm_init_state, ipm_set_state)
static void mark_fresh_state(ipm_handle* h) {
    h->haveState = true; h->predictor_valid = false; h->fresh_state = true;
    h->h_sc->status = 0;                                       // (a certificate describes the iterate of its detection only)
}

extern "C" int ipm_init_state_mehrotra(ipm_handle* h, int32_t* pivots_fixed) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "ipm_init_state_mehrotra: NULL handle");
    if (!h->haveA) return fail(h, IPM_ERR_STATE, "ipm_init_state_mehrotra: A not set");
    if (!h->haveBC) return fail(h, IPM_ERR_STATE, "ipm_init_state_mehrotra: (b, c) not set");
    if (int rc_ = compat_refuse(h, "ipm_init_state_mehrotra", IPM_FEATURE_MEHROTRA_START)) return rc_;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    for (int attempt = 0;; ++attempt) {                     // second pass only after a recovered poll time-out
        hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, 1e-8, 1e-8, 1e-8, h->opt.eta, 1 << 30, 1, 1);
        if (h->small) {
            const SmallItem it = small_item(h, 0, 0, 0);
            launch_small(SMALL_START_ROWS[step_variant(h).bounded], h->stream, &it, nullptr, 1);
            HIP_TRY(h, hipGetLastError());
        } else if ((rc = enqueue_mehrotra_start(h))) return rc;
        bool tmo = false;
        if ((rc = read_scalars(h, &tmo))) return rc;           // the one synchronisation
        if (!tmo) break;
        if (attempt) return fail(h, IPM_ERR_HIP, "hand-off time-out persists with stream events");
        poll_fallback(h);
    }
    if (pivots_fixed) *pivots_fixed = h->h_sc->fixed;
    mark_fresh_state(h);
    return IPM_OK;
}

extern "C" int ipm_iterate(ipm_handle* h, int32_t n_steps, ipm_stats* stats) {
    int rc = check_ready(h, "ipm_iterate");
    if (rc) return rc;
    if (n_steps < 0) return fail(h, IPM_ERR_INVALID_ARG, "n_steps < 0");
    if ((rc = rounds_check_path(h, h->mcc, "ipm_iterate"))) return rc;
    if ((rc = rounds_check_path(h, h->ref, "ipm_iterate"))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    h->predictor_valid = false;
    std::vector<hipEvent_t> evs;
    struct EvGuard {                                   // destroyed on every return path
        std::vector<hipEvent_t>& v;
        ~EvGuard() { for (auto& e : v) if (e) (void)hipEventDestroy(e); }
    } guard{evs};
    if (h->profiling) {
        evs.assign((size_t)EV_PER_IT * n_steps, nullptr);
        for (auto& e : evs) HIP_TRY(h, hipEventCreate(&e));
    }
    float ms = 0.f;
    const int reset_k = h->fresh_state ? 1 : 0;      // iteration count and history restart with a newly set iterate
    h->fresh_state = false;
    if (h->small && !h->profiling) {
        hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, 1e-8, 1e-8, 1e-8, h->opt.eta, 1 << 30, 1, reset_k);
        HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
        if ((rc = enqueue_small(h, n_steps, 0))) return rc;
        HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
        if ((rc = read_scalars(h))) return rc;
        HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
        fill_stats(h, stats, ms);
        return IPM_OK;
    }
    for (int attempt = 0;; ++attempt) {
        hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, 1e-8, 1e-8, 1e-8, h->opt.eta, 1 << 30, 1,
                           attempt == 0 ? reset_k : 0);
        if ((rc = rounds_start(h, h->mcc, attempt == 0 && reset_k))) return rc;
        if ((rc = rounds_start(h, h->ref, attempt == 0 && reset_k))) return rc;
        const bool guard_poll = may_poll(h) && n_steps > 0;
        if (guard_poll && (rc = enqueue_snapshot(h, 0))) return rc;
        HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
        for (int it = 0; it < n_steps; ++it)
            if ((rc = enqueue_iteration(h, h->profiling ? &evs[(size_t)it * EV_PER_IT] : nullptr))) return rc;
        // residuals + stop test of the state just reached: the statistics describe what ipm_get_state returns
        if ((rc = enqueue_residuals(h))) return rc;
        HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
        bool tmo = false;
        if ((rc = read_scalars(h, &tmo))) return rc;
        if (!tmo) break;
        // (at most two recoveries per call: the fused launch falls back to formation + look-ahead factorization, which still polls
        //  device counters, and that one to stream events)
        if (attempt >= 2 || !guard_poll) return fail(h, IPM_ERR_HIP, "hand-off time-out persists with stream events");
        poll_fallback(h);
        if ((rc = enqueue_snapshot(h, 1))) return rc;
    }
    HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    if (h->profiling && n_steps > 0) {
        double ph[4] = {0, 0, 0, 0};
        for (int it = 0; it < n_steps; ++it) {
            hipEvent_t* e = &evs[(size_t)it * EV_PER_IT];
            float f = 0.f, total = 0.f;
            (void)hipEventElapsedTime(&f, e[1], e[2]); ph[0] += f;
            if (h->profiling < 2) continue;
            (void)hipEventElapsedTime(&f, e[2], e[3]); ph[1] += f;
            float s1 = 0.f, s2 = 0.f;
            (void)hipEventElapsedTime(&s1, e[4], e[5]); (void)hipEventElapsedTime(&s2, e[6], e[7]); ph[2] += s1 + s2;
            (void)hipEventElapsedTime(&total, e[0], e[8]);
            float f12 = 0.f, f23 = 0.f;
            (void)hipEventElapsedTime(&f12, e[1], e[2]); (void)hipEventElapsedTime(&f23, e[2], e[3]);
            ph[3] += total - f12 - f23 - s1 - s2;
        }
        for (int i = 0; i < 4; ++i) h->phase_ms[i] = ph[i] / n_steps;
    }
    fill_stats(h, stats, ms);
    return IPM_OK;
}

extern "C" int ipm_solve(ipm_handle* h, double tol_p, double tol_d, double tol_gap, int32_t max_iter, ipm_stats* stats) {
    int rc = check_ready(h, "ipm_solve");
    if (rc) return rc;
    if (max_iter < 0) return fail(h, IPM_ERR_INVALID_ARG, "max_iter < 0");
    if ((rc = rounds_check_path(h, h->mcc, "ipm_solve"))) return rc;
    if ((rc = rounds_check_path(h, h->ref, "ipm_solve"))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    h->predictor_valid = false; h->fresh_state = false;
    if (h->auto_reg) { h->auto_reg = 0; h->shift_rel = h->opt.regularize; }      // decided per solve
    hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, tol_p, tol_d, tol_gap, h->opt.eta, max_iter, 0, 1);
    if ((rc = rounds_start(h, h->mcc, true))) return rc;
    if ((rc = rounds_start(h, h->ref, true))) return rc;
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    const int chunk = h->opt.check_every;
    const bool may_auto = h->opt.regularize == 0.0 && !(h->opt.flags & IPM_FLAG_NO_AUTO_REGULARIZE);
    if (h->small) {
        // one launch runs the loop to its end; a second one only when the first factorization asked for the shift
        // (the kernel leaves before it touches the iterate, so there is nothing to roll back)
        if ((rc = enqueue_small(h, 1 << 30, may_auto ? 1 : 0))) return rc;
        if ((rc = read_scalars(h))) return rc;
        if (h->h_sc->status == IPM_STATUS_NEEDS_SHIFT) {
            h->shift_rel = 1e-14; h->auto_reg = 1;
            hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, tol_p, tol_d, tol_gap, h->opt.eta, max_iter, 0, 1);
            if ((rc = enqueue_small(h, 1 << 30, 0))) return rc;
            if ((rc = read_scalars(h))) return rc;
        }
        HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
        HIP_TRY(h, hipEventSynchronize(h->ev1));
        float ms_ = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms_, h->ev0, h->ev1));
        fill_stats(h, stats, ms_);
        return IPM_OK;
    }
    bool first = true;
    int recovered = 0;
    for (;;) {
        // roll-back point: the first chunk (auto-regularize restart) and every chunk that can hit a poll time-out
        const bool snap = first || may_poll(h);
        if (snap && (rc = enqueue_snapshot(h, 0))) return rc;
        for (int i = 0; i < chunk; ++i)
            if ((rc = enqueue_iteration(h, nullptr))) return rc;
        bool tmo = false;
        if ((rc = read_scalars(h, &tmo))) return rc;
        if (tmo) {
            if (!snap || ++recovered > 2) return fail(h, IPM_ERR_HIP, "hand-off time-out persists with stream events");
            poll_fallback(h);
            if ((rc = enqueue_snapshot(h, 1))) return rc;
            continue;                                          // same chunk again, with stream events
        }
        if (first && may_auto && h->h_sc->k > 0 && (double)h->h_sc->fixed_first > 0.05 * (double)h->m) {
            // A has > 5 % dependent rows (QAP family): the guard alone stalls the loop.  Restart
            // this solve from its start state with the 1e-14 Tikhonov shift.  No other Netlib file crosses 2.7 %, so
            // every solve that does not take this branch is bit-identical to one with the flag off.
            h->shift_rel = 1e-14; h->auto_reg = 1;
            if ((rc = enqueue_snapshot(h, 1))) return rc;
            first = false;
            continue;
        }
        first = false;
        if (h->h_sc->done) break;
    }
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    float ms = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    fill_stats(h, stats, ms);
    return IPM_OK;
}
