// The three train paths that work in sample space -- the table formulation, Phi-free with fp32
// affinities, and the streamed fp64 form -- with what they share (the Sinkhorn iterations on the p-sized side, the host route
// of the orthogonalisation), the TableFilter members, V on demand and apply on the p-sized side of a table filter.
#include "train.h"

using namespace nlep;

namespace {
// Operands of the factored Sinkhorn update (fused.hip: k_sink_update_a/b) from what solve_Ka left: X1 (2p x r column-major)
// and X2 (2p x r row-major) = [B; V_A], lambda.
void build_update_operands(nle_ctx* c, const Nystrom& ny, int p, DevBuf<double>& d_X1, DevBuf<double>& d_X2,
                           DevBuf<double>& d_lam) {
    const int r = ny.r;
    if (ny.dev) {
        // Cholesky form with the factors on the device: X1 = [L^-T; 0] (2p x p column-major), X2 = [L^-T; Ka] row-major --
        // row a of L^-T is column a of L^-1 and Ka is symmetric, so X2 is two plain copies and X1 one transpose
        const size_t n2 = (size_t)2 * p, pp = (size_t)p * p;
        d_X1.alloc(n2 * p);
        d_X2.alloc(n2 * p);
        d_lam.alloc(p);
        HIP_OK(hipMemsetAsync(d_X1.p, 0, n2 * p * sizeof(double), c->stream));
        HIP_OK(nlek::transpose64(c->stream, p, ny.dev->ch.Linv.p, d_X1.p, p, 2 * p));
        HIP_OK(hipMemcpyAsync(d_X2.p, ny.dev->ch.Linv.p, pp * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(d_X2.p + pp, ny.dev->Ka.p, pp * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIP_OK(nlek::fill64(c->stream, d_lam.p, p, 1.0));
    } else {
        // X1 (2p x r column-major) and X2 (2p x r row-major) = [B; V_A]; Cholesky form: X1 = [L^-T; 0], the lower
        // half of X2 = the rows of Ka itself (exact projector / exact V_A diag(lambda) V_A^T, see k_sink_update_b)
        const size_t n2 = (size_t)2 * p;
        std::vector<double> X1(n2 * r, 0.0), X2(n2 * r);
        for (int k = 0; k < r; ++k)
            for (int a = 0; a < p; ++a) {
                const double b = ny.B[(size_t)k * p + a];
                const double va = ny.chol ? ny.Ka[(size_t)k * p + a] : ny.VA[(size_t)k * p + a];  // Ka symmetric
                X1[(size_t)k * n2 + a] = b;
                if (!ny.chol) X1[(size_t)k * n2 + p + a] = va;
                X2[(size_t)a * r + k] = b;
                X2[(size_t)(p + a) * r + k] = va;
            }
        d_X1.alloc(X1.size());
        d_X2.alloc(X2.size());
        d_lam.alloc(r);
        HIP_OK(hipMemcpyAsync(d_X1.p, X1.data(), X1.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(d_X2.p, X2.data(), X2.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(d_lam.p, ny.lam.data(), r * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));  // the staging vectors go out of scope (the column-sum pass is done by now)
    }
}

// The Sinkhorn iterations in sample space (reference :238-245 as 2T passes), shared by the table / Phi-free and the
// streamed fp64 formulations.  Each pass has an N-sized half, the caller's pass_pixels(mode, last) -- z = the column sums
// over this rank's pixels under the scaling whose sample-side vector is d_w; the last pass also stores its row scalings c
// -- and a p-sized half here: the all-reduce of z (zrows slices of stride zld), then the factored update (fused.hip).
// Pass n uses the scaling whose sample row sums are sAh[n-1] (and w) and produces sAh[n]; pass 0 is the column sum
// Phi^T 1 (:234,239).  The constructor makes d_w (zero: the pass kernels read its padding up to zld), so it goes where
// the caller's launch order wants that memset.
struct SampleSinkhorn {
    nle_ctx* c;
    int p, T, zld;
    DevBuf<double> d_w, d_sAh, d_X1, d_X2, d_lam, d_uv;
    // sample row sums V_A u of the scaling that defines the final c (input of the last pass) and of the output of the
    // last pass (the r scaling): complete once the stream is drained after run()
    std::vector<double> sA_c, sA_r;
    double* h_sA = nullptr;  // run(defer): the two, staged (page-locked) until fetch_row_sums()

    SampleSinkhorn(nle_ctx* c_, int p_, int zld_, int T_)
        : c(c_), p(p_), T(T_), zld(zld_), d_w(zld_), d_sAh((size_t)2 * T_ * p_), d_uv((size_t)3 * p_) {
        HIP_OK(hipMemsetAsync(d_w.p, 0, zld * sizeof(double), c->stream));
    }

    // `solve` factors Ka on the host (solve_Ka); it is called only after the first pass -- the column sum, which needs
    // nothing of it -- is on the stream, so the factorisation runs under that pass.
    // `defer` (single rank, W_A's root on the host: train_tables): sA_c and sA_r go to the ctx's staging block with the
    // hand-over event behind them instead, so that the caller can queue the Gram stage before it waits -- for the event
    // alone, in fetch_row_sums().  Without room in the staging block the copies are today's.
    Nystrom run(const SolveKa& solve, const std::function<void(int, bool)>& pass_pixels, double* d_z, int zrows,
                bool defer = false) {
        pass_pixels(nlek::ROWPASS_COLSUM, false);
        Nystrom ny = solve();
        build_update_operands(c, ny, p, d_X1, d_X2, d_lam);
        auto update = [&](int n, int mode) {
            all_reduce(c, d_z, (size_t)zrows * zld);
            PROFILED(c, NLE_K_SMALL,
                     nlek::sink_update(c->stream, mode, p, ny.r, ny.chol, d_X1.p, d_X2.p, d_lam.p, d_z, zrows, zld,
                                       n > 0 ? d_sAh.p + (size_t)(n - 1) * p : nullptr, NLE_EPS, d_uv.p, d_uv.p + 2 * p,
                                       d_sAh.p + (size_t)n * p, d_w.p));
        };
        update(0, nlek::ROWPASS_COLSUM);
        for (int n = 1; n < 2 * T; ++n) {
            pass_pixels(nlek::ROWPASS_RECIP, n == 2 * T - 1);
            update(n, nlek::ROWPASS_RECIP);
        }
        // (Fetching these on a second stream, so that the Gram kernels could be queued first, saved ~50 us but made two
        // processes sharing one GPU stall for tens of milliseconds per all-reduce: one stream per ctx it stays.)
        sA_c.resize(p);
        sA_r.resize(p);
        // (Cholesky form of Ka only: the other uploads V_A and waits for Kr ahead of the Gram kernels, ortho.hip)
        if (defer && ny.chol && !wa_root_on_device(c, ny.r)) h_sA = static_cast<double*>(pinned_take(c, (size_t)2 * p * sizeof(double)));
        if (h_sA) {  // the two vectors are neighbours in d_sAh: one copy
            HIP_OK(hipMemcpyAsync(h_sA, d_sAh.p + (size_t)(2 * T - 2) * p, (size_t)2 * p * sizeof(double), hipMemcpyDeviceToHost,
                                  c->stream));
            HIP_OK(hipEventRecord(handover_event(c), c->stream));
            return ny;
        }
        HIP_OK(hipMemcpyAsync(sA_c.data(), d_sAh.p + (size_t)(2 * T - 2) * p, p * sizeof(double), hipMemcpyDeviceToHost,
                              c->stream));
        HIP_OK(hipMemcpyAsync(sA_r.data(), d_sAh.p + (size_t)(2 * T - 1) * p, p * sizeof(double), hipMemcpyDeviceToHost,
                              c->stream));
        return ny;
    }

    bool deferred() const { return h_sA != nullptr; }
    // deferred: wait for the staged copy -- not for what the caller has queued behind it -- and take the two vectors
    void fetch_row_sums() {
        handover_wait(c->hand_ev);
        std::copy(h_sA, h_sA + p, sA_c.begin());
        std::copy(h_sA + p, h_sA + 2 * p, sA_r.begin());
        h_sA = nullptr;
    }
};

// The host route of the sample-space orthogonalisation, the part that does not need the Gram under the Gram kernels.  The
// fp32 Phi-free form always takes it, the table form with the opt-in Lanczos solver: that one works on the LITERAL q x q
// matrix Q = Wa + S (Wab Wab^T) S with Wa as computed, not mirrored from its lower triangle -- what Spectra's
// DenseGenMatProd multiplies by in a USE_SPECTRA build, src/filter.cpp:174, 311 -- which the host forms exactly; the device
// route diagonalises a symmetric similar matrix.  d_G: what enqueue_gram fills, 16 x 16 upper tiles (gram64) or p x p.
OrthoSS ortho_ss_host(nle_ctx* c, const Nystrom& ny, int p, const SampleSinkhorn& sk, const std::function<void()>& enqueue_gram,
                      double* d_G, size_t g_elems, bool tile16, int n_eig, Timer& tm_g, double* host_ms, Trace& tr) {
    OrthoSS o;
    enqueue_gram();
    // host, while the Gram kernel runs
    ortho_ss_prepare(o, ny, p, sk.sA_c, sk.sA_r, /*literal_q=*/c->topk_solver != 0, c->sw.force_eig, tr.on);
    tr.mark("ss: ortho prepare (host)");
    // (a device-to-host copy into pageable memory blocks the host until the stream reaches it, so it
    // is issued only now)
    all_reduce(c, d_G, g_elems);
    std::vector<double> tiles(g_elems);
    HIP_OK(hipMemcpyAsync(tiles.data(), d_G, tiles.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    tm_g.stop();
    HIP_OK(hipStreamSynchronize(c->stream));
    tr.mark("ss: gram sync");
    const double h0 = now_ms();
    ortho_ss_finish(o, tile16 ? unpack_tiles(tiles, nlek::gram64_ld(p), p, 16) : std::move(tiles), n_eig, c->topk_solver, tr.on);
    *host_ms += now_ms() - h0;
    tr.mark("ss: ortho finish (host)");
    return o;
}

}  // namespace

// X (p x K column-major on the host) as the p x ldd row-major, zero-padded operand of project64 / k_apply_small
std::vector<double> nlep::padded_rows(const std::vector<double>& X, int p, int K, int ldd) {
    std::vector<double> R((size_t)p * ldd, 0.0);
    for (int k = 0; k < K; ++k)
        for (int a = 0; a < p; ++a) R[(size_t)a * ldd + k] = X[(size_t)k * p + a];
    return R;
}

// quantised luminance + Cartesian sample grid: table look-ups replace the exponentials (tables.hip), and the pixel halves of
// every table pass run on level-sorted rows, without LDS atomics (sorted.hip; sorted once here).  d_lum: virtual full base.
// Which form each sorted kernel takes is decided here and nowhere else: sorted.hip's bounds on the bandwidth, and the
// switches of the call's snapshot that force a plain form.
nlep::TableFilter::TableFilter(nle_ctx* ctx, const float* d_lum, const SampleSet& ss, double hx, double hy, int row0_, int nrows_)
    : gs(ss.gs), p(ss.p), P64(nlek::sink_pass_ld(ss.p)), row0(row0_), nrows(nrows_), nsw(nsw_of(hx)), npw(nsw_of(hy)),
      lum(d_lum), samples(upload_samples(ctx, ss, nlek::sink_pass_ld(ss.p))), c((size_t)nrows_ * ss.gs.W),
      er((size_t)nrows_ * ss.gs.nSelRows), ecT((size_t)ss.gs.nSelCols * ss.gs.W), Ep((size_t)256 * ss.p),
      sample_loc((size_t)ss.p) {
    {  // the samples' pixel index within this rank's rows (-1: another rank's): known before the first kernel
        const long long pix0 = (long long)row0_ * ss.gs.W, M = (long long)nrows_ * ss.gs.W;
        h_sample_loc.resize(p);
        for (int a = 0; a < p; ++a) {
            const long long loc = ss.pix[a] - pix0;
            h_sample_loc[a] = (loc >= 0 && loc < M) ? loc : -1;
        }
        HIP_OK(hipMemcpyAsync(sample_loc.p, h_sample_loc.data(), p * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    }
    PROFILED(ctx, NLE_K_SMALL, nlek::hist_tables(ctx->stream, gs, samples.p, p, hx, hy, row0, nrows, er.p, ecT.p, Ep.p));
    const nlesw::Switches& sw = ctx->sw;
    if (gs.W > nlek::sorted_max_width() || sw.no_sorted_rows) return;
    scol.alloc(nlek::sorted_scol_elems(gs.W, nrows));  // k_sort_rows writes every entry a pass reads
    first.alloc((size_t)nrows * 258);
    desc.alloc((size_t)nrows * nlek::kSortedThreads);
    E.alloc((size_t)gs.W + 1);
    PROFILED(ctx, NLE_K_SMALL, nlek::dist_table(ctx->stream, gs.W, hx, E.p));
    // single rank: training will leave apply's reduce half for this plane (train_tables), which needs the plane kept in a
    // form apply can compare its input with -- one byte per pixel, written by the sort
    if (ctx->world == 1 && !ctx->comm && ctx->train_reduce) lev.alloc((size_t)nrows * gs.W);
    PROFILED(ctx, NLE_K_SMALL, nlek::sort_rows(ctx->stream, d_lum, gs, row0, nrows, scol.p, desc.p, first.p, lev.p));
    HIP_OK(hipMemsetAsync(c.p, 0, c.n * sizeof(double), ctx->stream));  // sample pixels are never visited
    sorted = nlek::SortedRows{scol.p, desc.p, first.p, E.p, false, 0.0};
    sorted.rec = nlek::sorted_recurrence(gs, hx, &sorted.kappa) && !sw.sorted_table;  // (kappa is set either way)
    sorted.mom = nlek::sorted_moments_ok(gs, hx) && !sw.sorted_table && !sw.sorted_no_moments;
    sorted.wgs_per_cu = sw.sorted_wgs_per_cu;
    if (!sw.all_level_tiles) {  // the tables' columns of level tiles that do not occur are skipped
        int t0 = 0, t1 = 16;
        while (t0 < 15 && !((ss.level_tiles >> t0) & 1u)) ++t0;
        while (t1 > t0 + 1 && !((ss.level_tiles >> (t1 - 1)) & 1u)) --t1;
        sorted.lev_t0 = t0;
        sorted.lev_nt = t1 - t0;
    }
    if (nlek::sorted_gsum_ok(gs, hx) && !sw.gram_pairs) {  // the Gram on index sums: one more distance table, exp(-2 d^2 / hx^2)
        E2.alloc((size_t)gs.W + 1);
        PROFILED(ctx, NLE_K_SMALL, nlek::dist_table(ctx->stream, gs.W, hx / std::sqrt(2.0), E2.p));
        sorted.E2 = E2.p;
        sorted.hx = hx;
    }
}

// The training plane for the consumers that read it after training (V on demand).  On the level-sorted path it was not
// kept: plane_into rebuilds this rank's rows from the sorted rows and the sample values into `dst` -- exact, the plane is
// integer valued -- and returns the virtual base of the full image; where the plane is held it returns that and leaves
// `dst` alone.  ensure_plane keeps the rebuilt rows in `slab` (V is being materialised: 4 bytes per pixel beside 4 K).
const float* nlep::TableFilter::plane_into(nle_ctx* ctx, DevBuf<float>& dst) const {
    if (lum || !sorted_rows() || nrows <= 0) return lum;
    dst.alloc((size_t)nrows * gs.W);
    PROFILED(ctx, NLE_K_SMALL, nlek::rows_from_sorted(ctx->stream, gs, row0, nrows, sorted, samples.p, p, dst.p));
    return dst.p - (long long)row0 * gs.W;
}
void nlep::TableFilter::ensure_plane(nle_ctx* ctx) { lum = plane_into(ctx, slab); }

namespace nlep {

// (2) the table formulation: every N-sized pass works on look-up tables of the quantised plane; V
// stays implicit (TableFilter)
void TrainPath::train_tables(const SolveKa& solve) {
    const int p = ss.p;
    tm_s.start();
    auto t = std::make_unique<TableFilter>(c, d_lum, ss, hx, hy, (int)(pix0 / ss.gs.W), (int)(M / ss.gs.W));
    const nlek::TableView view = t->view();
    DevBuf<double> d_z(t->P64), d_hws(nlek::hist_tiled_workspace_elems(ss.gs, t->nrows));
    SampleSinkhorn sk(c, p, t->P64, T);
    tr.mark("ss: alloc+upload");
    auto pass_pixels = [&](int mode, bool last) {  // the N-sized half: the local column sums, straight into d_z
        ProfObserver obs(c, kProfTablePass);
        HIP_OK(nlek::sink_hist_tiled(c->stream, mode, view, sk.d_w.p, NLE_EPS, last ? t->c.p : nullptr, d_hws.p, d_z.p, &obs));
    };
    // Single rank with the full eigensolve of Q: neither the Gram kernels nor the reduce half read anything the host computes
    // after the last pass, so they are queued before the host waits for the last pass's row sums (run(defer); the host
    // route of W_A's root only) -- every launch the host makes in front of that root is on the critical path.
    const Nystrom ny = sk.run(solve, pass_pixels, d_z.p, 1, /*defer=*/c->world == 1 && !c->comm && c->topk_solver == 0);
    const bool gram_first = sk.deferred();
    adopt_nystrom(f, ny, NLE_MODE_PHI_FREE);
    tm_s.stop();
    tr.mark("ss: passes enqueued");
    if (!gram_first) {
        HIP_OK(hipStreamSynchronize(c->stream));
        tr.mark("ss: sinkhorn sync");
    }

    // Gram in sample space: histogram + fp64 GEMM over the look-up tables (k_ghist_*), enqueued; the host half that does
    // not need it runs meanwhile
    tm_g.start();
    const size_t g_elems = (size_t)p * p;
    DevBuf<double> d_gpart, d_G(g_elems);
    auto enqueue_gram = [&] {
        d_gpart.alloc(nlek::ghist_workspace_elems(ss.gs, t->nrows));
        {
            ProfObserver obs(c, kProfTableGram);
            HIP_OK(nlek::gram_hist(c->stream, view, d_gpart.p, d_G.p, &obs));
        }
        // The reduce half of apply for the plane in hand, m = K^T (c o x): it needs the row scalings and the plane, nothing
        // that comes after the Sinkhorn iterations, and `enhance` filters the plane it trained on.  Behind the Gram kernels
        // the stream is idle while the host takes Wa apart, so it runs here, off the critical path -- apply_sample_space's
        // own launches with its arguments, so the bits are the ones apply would compute (d_hws is free by now).
        if (t->lev.p) {
            t->m_train.alloc(t->P64);
            t->xA_train.alloc(p);
            {
                ProfObserver obs(c, kProfTableReduce);
                HIP_OK(nlek::sink_hist_tiled(c->stream, nlek::ROWPASS_XVEC, view, nullptr, NLE_EPS, nullptr, d_hws.p,
                                             t->m_train.p, &obs, d_lum));
            }
            PROFILED(c, NLE_K_SMALL, nlek::gather_sample_levels(c->stream, t->lev.p, ss.gs, t->row0, t->nrows, t->xA_train.p));
        }
    };
    // what defines V = diag(c) K_AB^T D implicitly (K' <= 128: tables_apply) stays on the device: D and the exact rows of V
    // at the sample pixels, p x ldd row-major, zero padded -- the operands of k_apply_small and project64
    auto place = [&](int K) {
        t->ldd = nlek::project64_ld(K);
        const size_t n = (size_t)p * t->ldd;
        t->D.alloc(n);
        t->Vrows.alloc(n);
        HIP_OK(hipMemsetAsync(t->D.p, 0, n * sizeof(double), c->stream));
        HIP_OK(hipMemsetAsync(t->Vrows.p, 0, n * sizeof(double), c->stream));
        return DeviceDV{t->D.p, t->Vrows.p, t->ldd};
    };
    if (gram_first) {
        enqueue_gram();
        tr.mark("ss: gram enqueued");
        sk.fetch_row_sums();
        tr.mark("ss: sinkhorn sync");
    }
    OrthoSS o;  // (outlives the last synchronisation below: o.staged)
    if (c->topk_solver == 0) {
        // the q-sized products run on the device, the eigensolves on the host; D and Vrows are written where apply reads
        // them and never visit the host
        ortho_ss_device(c, o, ny, p, sk.sA_c, sk.sA_r, d_G.p, n_eig,
                        gram_first ? std::function<void()>() : std::function<void()>(enqueue_gram),
                        [&] { all_reduce(c, d_G.p, g_elems); }, host_ms, tr, place);
        tm_g.stop();
    } else {
        o = ortho_ss_host(c, ny, p, sk, enqueue_gram, d_G.p, g_elems, /*tile16=*/false, n_eig, tm_g, host_ms, tr);
    }
    adopt_ortho(f, o);

    tm_p.start();
    std::vector<double> Dp, Vr;  // host route only: staged until the synchronisation below
    if (c->topk_solver != 0) {
        const DeviceDV dst = place(o.K);
        Dp = padded_rows(o.D, p, o.K, dst.ldd), Vr = padded_rows(o.Vrows, p, o.K, dst.ldd);
        HIP_OK(hipMemcpyAsync(dst.D, Dp.data(), Dp.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(dst.Vrows, Vr.data(), Vr.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    // the caller's plane is not ours to keep.  With level-sorted rows nothing on the apply path reads the plane, and the
    // rows hold it exactly: it is rebuilt if V is ever asked for (TableFilter::ensure_plane).  Without them the unsorted
    // kernels read it in every apply: keep a copy of this rank's rows.
    if (t->sorted_rows()) {
        t->lum = nullptr;
    } else {
        t->slab.alloc((size_t)M);
        HIP_OK(hipMemcpyAsync(t->slab.p, d_lum + pix0, (size_t)M * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        t->lum = t->slab.p - pix0;
    }
    t->drop_gram_only();
    f->tables = std::move(t);
    tm_p.stop();
    // the one synchronisation after eig(Q): the filter is valid from here, and o.staged / Dp / Vr may go.  (On the stream and
    // not left to the timers' hipEventSynchronize: with that wait alone the gap from the last product to apply's first copy
    // was 176 us, with this one 101 us: profiles/r10_handover.txt, section 2)
    HIP_OK(hipStreamSynchronize(c->stream));
}

// (2b) Phi-free with fp32 affinities (NLE_MODE_PHI_FREE on a plane that is not integer valued, NLE_MODE_PHI_FREE_EXP): every
// N-sized pass regenerates its affinity rows (fused.hip)
void TrainPath::train_phi_free_exp(const SolveKa& solve) {
    const int p = ss.p;
    if (p > nlek::sink_pass_max_p()) throw Fail{NLE_ERR_INVALID, "Phi-free path: too many samples for the generic kernels"};
    const int P64 = nlek::sink_pass_ld(p);
    const float nsw = nsw_of(hx), npw = nsw_of(hy);
    tm_s.start();
    // the pass kernel reads the sample table up to the next multiple of 16: pad with zeros (their
    // w entries are zero, so they only have to be finite)
    DevBuf<float4> d_samples = upload_samples(c, ss, P64);
    constexpr int kZS = 8;  // slices of the block partials, summed by k_sink_update
    const int npart = nlek::sink_pass_rows(M);  // M > 0: every rank owns an image row (train_impl)
    DevBuf<double> d_z((size_t)kZS * P64), d_partial((size_t)npart * P64), d_cbuf((size_t)M);
    SampleSinkhorn sk(c, p, P64, T);
    tr.mark("ss: alloc+upload");
    auto pass_pixels = [&](int mode, bool last) {  // the N-sized half: z = sum over this rank's pixels
        PROFILED(c, NLE_K_SINKHORN_PASS, nlek::sink_pass(c->stream, mode, d_lum, ss.gs, d_samples.p, p, sk.d_w.p, nsw, npw, pix0,
                                                         M, NLE_EPS, last ? d_cbuf.p : nullptr, d_partial.p));
        PROFILED(c, NLE_K_REDUCE, nlek::reduce_partials(c->stream, d_partial.p, npart, P64, d_z.p, kZS));
    };
    const Nystrom ny = sk.run(solve, pass_pixels, d_z.p, kZS);
    adopt_nystrom(f, ny, NLE_MODE_PHI_FREE_EXP);
    tm_s.stop();
    tr.mark("ss: passes enqueued");
    HIP_OK(hipStreamSynchronize(c->stream));
    tr.mark("ss: sinkhorn sync");

    // Gram in sample space on regenerated affinity rows (k_gram64, fp64 MFMA), enqueued; the host half that does not need
    // it runs meanwhile
    tm_g.start();
    const size_t g_elems = (size_t)nlek::gram64_num_tiles(p) * 256;
    DevBuf<double> d_gpart(nlek::gram64_partial_elems(M, p)), d_tiles(g_elems);
    auto enqueue_gram = [&] {
        PROFILED(c, NLE_K_GRAM, nlek::gram64(c->stream, d_lum, ss.gs, d_samples.p, p, nsw, npw, pix0, M, d_cbuf.p, d_gpart.p,
                                             d_tiles.p));
    };
    const OrthoSS o = ortho_ss_host(c, ny, p, sk, enqueue_gram, d_tiles.p, g_elems, /*tile16=*/true, n_eig, tm_g, host_ms, tr);
    adopt_ortho(f, o);

    // V = diag(c) K_AB^T D: the Nystrom extension of the K' <= 128 (train_impl) retained eigenvectors, affinity fused
    tm_p.start();
    const std::vector<double> Dp = padded_rows(o.D, p, o.K, nlek::project64_ld(o.K));
    DevBuf<double> d_D(Dp.size());
    HIP_OK(hipMemcpyAsync(d_D.p, Dp.data(), Dp.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    DevBuf<float> d_V((size_t)M * f->ldv);
    PROFILED(c, NLE_K_PROJECT, nlek::project64(c->stream, d_lum, ss.gs, d_samples.p, p, nsw, npw, pix0, M, d_D.p, o.K,
                                               d_cbuf.p, d_V.p, f->ldv));
    tr.mark("ss: project enqueued");
    scatter_sample_rows(c, ss.pix, p, o.Vrows, o.K, f->ldv, pix0, M, d_V.p);
    tm_p.stop();
    HIP_OK(hipStreamSynchronize(c->stream));
    tr.mark("ss: project sync");
    f->V = std::move(d_V);
}

// (3) The same sample-space algebra on fp64 affinity rows (k_affinity64: libm exp of the reference's own argument, :104-112),
// regenerated CHUNK BY CHUNK in every pass: no N x r matrix, a bounded workspace, any luminance plane, any grid up to 2048
// samples, any K.  Every N-sized step is a generic64.hip kernel on the chunk (k_i = row i of the chunk):
//   Sinkhorn half-iteration   y_i = recip(k_i . w), z += k_i y_i                 k_rowpass64 (u := w)
//   Gram                      Gk += sum c_i^2 k_i k_i^T                          k_gram64d
//   eigenvectors              V_i = c_i k_i^T D                                  k_tsgemm64      (V: N x K' fp64, as mode 4)
// and the p-sized side is train_tables' (SampleSinkhorn, ortho_ss_device).  Costs a pass 2 x N p 8 bytes of HBM
// traffic (write + read of the chunk) where the materialised form reads N r 8 once -- the price of not holding it.
void TrainPath::train_stream64(const SolveKa& solve) {
    const int p = ss.p, ld = ld4(p);
    hipStream_t st = c->stream;
    tm_s.start();
    const size_t budget_mb = (size_t)c->sw.stream64_chunk_mb;
    const long long rows_fit = (long long)((budget_mb << 20) / ((size_t)ld * sizeof(double)));
    const long long CH = std::max<long long>(256, std::min<long long>(std::max<long long>(M, 1), rows_fit));
    const AffinityRows64 kab(c, d_lum, ss, hx, hy, /*want_mask=*/true);
    DevBuf<double> d_K((size_t)CH * ld), d_partial((size_t)nlek::kRowpassMaxBlocks * ld), d_zc(ld), d_z(ld), d_ones(ld),
        d_cbuf((size_t)std::max<long long>(M, 1));
    SampleSinkhorn sk(c, p, ld, T);
    HIP_OK(nlek::fill64(st, d_ones.p, ld, 1.0));
    tr.mark("s64: alloc+upload");
    auto chunk_rows = [&](long long i0) { return std::min<long long>(CH, M - i0); };
    auto gen = [&](long long i0, long long mc) { PROFILED(c, NLE_K_AFFINITY, kab.rows(pix0 + i0, mc, d_K.p, true)); };
    auto pass_pixels = [&](int mode, bool last) {
        HIP_OK(hipMemsetAsync(d_z.p, 0, ld * sizeof(double), st));
        for (long long i0 = 0; i0 < M; i0 += CH) {
            const long long mc = chunk_rows(i0);
            gen(i0, mc);
            int nb = 0;
            PROFILED(c, NLE_K_SINKHORN_PASS, nlek::rowpass64(st, mode, d_K.p, mc, ld, ld, sk.d_w.p, d_ones.p, nullptr, NLE_EPS, d_partial.p, &nb));
            PROFILED(c, NLE_K_REDUCE, nlek::reduce_partials(st, d_partial.p, nb, ld, d_zc.p));
            HIP_OK(nlek::add64(st, d_z.p, d_zc.p, ld));
            if (last) PROFILED(c, NLE_K_SMALL, nlek::row_scalings64(st, d_K.p, mc, ld, p, sk.d_w.p, NLE_EPS, d_cbuf.p + i0));
        }
    };
    const Nystrom ny = sk.run(solve, pass_pixels, d_z.p, 1);
    adopt_nystrom(f, ny, NLE_MODE_STREAMED_F64);
    tm_s.stop();
    HIP_OK(hipStreamSynchronize(st));
    tr.mark("s64: sinkhorn");
    // Gram: Gk = sum over the non-sample pixels of c_i^2 k_i k_i^T, chunk by chunk
    tm_g.start();
    const size_t pp = (size_t)p * p;
    DevBuf<double> d_G(pp), d_Gc(pp), d_gpart(std::max<size_t>(nlek::gram64d_partial_elems(CH, p), 1));
    auto enqueue_gram = [&] {
        HIP_OK(hipMemsetAsync(d_G.p, 0, pp * sizeof(double), st));
        for (long long i0 = 0; i0 < M; i0 += CH) {
            const long long mc = chunk_rows(i0);
            gen(i0, mc);
            PROFILED(c, NLE_K_GRAM, nlek::gram64d(st, d_K.p, mc, ld, p, d_cbuf.p + i0, d_gpart.p, d_Gc.p));
            HIP_OK(nlek::add64(st, d_G.p, d_Gc.p, pp));
        }
    };
    OrthoSS o;
    ortho_ss_device(c, o, ny, p, sk.sA_c, sk.sA_r, d_G.p, n_eig, enqueue_gram, [&] { all_reduce(c, d_G.p, pp); }, host_ms, tr);
    tm_g.stop();
    adopt_ortho(f, o);
    // V = diag(c) K D (the Nystrom extension of the K' kept eigenvectors, :324-327) + the exact sample rows
    tm_p.start();
    DevBuf<double> d_D((size_t)p * o.K), d_V((size_t)std::max<long long>(M, 1) * f->ldv);
    HIP_OK(hipMemcpyAsync(d_D.p, o.D.data(), o.D.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_V.p, 0, d_V.n * sizeof(double), st));
    for (long long i0 = 0; i0 < M; i0 += CH) {
        const long long mc = chunk_rows(i0);
        gen(i0, mc);
        PROFILED(c, NLE_K_PROJECT, nlek::ts_gemm64(st, d_K.p, mc, ld, p, d_D.p, o.K, d_cbuf.p + i0, d_V.p + (size_t)i0 * f->ldv, f->ldv));
    }
    scatter_sample_rows(c, ss.pix, p, o.Vrows, o.K, f->ldv, pix0, M, d_V.p);
    tm_p.stop();
    HIP_OK(hipStreamSynchronize(st));
    tr.mark("s64: project");
    f->V64 = std::move(d_V);
}

// the exact sample rows of V of a table filter on the host, p x K column-major (scatter_sample_rows' operand), fetched from
// the device: only V on demand reads them
std::vector<double> host_Vrows(const nle_filter* f) {
    nle_ctx* c = f->ctx;
    const TableFilter& t = *f->tables;
    std::vector<double> rows((size_t)t.p * t.ldd), out((size_t)t.p * f->K);
    HIP_OK(hipMemcpyAsync(rows.data(), t.Vrows.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < f->K; ++k)
        for (int a = 0; a < t.p; ++a) out[(size_t)k * t.p + a] = rows[(size_t)a * t.ldd + k];
    return out;
}

// materialise V = diag(c) K D of a table filter (projection kernel + exact sample rows)
void ensure_V(nle_filter* f) {
    if (f->V.p || (!f->V64.p && !f->tables)) return;
    nle_ctx* c = f->ctx;
    const long long M = f->n_local, pix0 = (long long)f->row0 * f->W;
    DevBuf<float> d_V((size_t)std::max<long long>(M, 1) * f->ldv);
    if (f->V64.p) {  // fp64 formulation: an fp32 copy for the accessors that hand out float pointers
        HIP_OK(nlek::to_f32(c->stream, f->V64.p, M * f->ldv, d_V.p));
    } else {
        f->tables->ensure_plane(c);
        const TableFilter& t = *f->tables;
        PROFILED(c, NLE_K_PROJECT, nlek::project64(c->stream, t.lum, t.gs, t.samples.p, t.p, t.nsw, t.npw, pix0, M, t.D.p, f->K,
                                                   t.c.p, d_V.p, f->ldv));
        scatter_sample_rows(c, f->h_sample_pix, f->p, host_Vrows(f), f->K, f->ldv, pix0, M, d_V.p);
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    f->V = std::move(d_V);
}

// apply on the p-sized side of a table filter: reduce half (column sums m = sum_i k_i c_i x_i through the
// tables), the p/K-sized middle (k_apply_small), and one table pass per output layer
void apply_sample_space(nle_filter* f, const float* d_x, const double* h_g /* L x K */, int L, float* d_y,
                        const LayersDone& done, int group, bool round8, long long ystride) {
    nle_ctx* c = f->ctx;
    const TableFilter& t = *f->tables;
    const nlek::TableView view = t.view();
    const long long M = ystride > 0 ? ystride : f->n_local;  // stride of the output layers
    const int p = t.p, K = f->K, P64 = t.P64;
    DevBuf<double> d_ws(nlek::hist_tiled_workspace_elems(t.gs, t.nrows)), d_m(P64), d_resp((size_t)L * K), d_t(K),
        d_Wp((size_t)L * P64), d_YA((size_t)L * p);
    HIP_OK(hipMemcpyAsync(d_resp.p, h_g, (size_t)L * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // The plane training left its reduce half for (TableFilter::m_train)?  Decided by content, not by pointer, and on the
    // device: one streaming pass over x against the kept level plane sets d_differs, the reduce kernels return at once
    // where it stays 0, and k_apply_small then reads training's m and sample values -- no verdict travels to the host.
    DevBuf<int> d_differs;
    if (t.m_train.p && c->world == 1 && !c->comm && c->train_reduce) {
        d_differs.alloc(1);
        HIP_OK(hipMemsetAsync(d_differs.p, 0, sizeof(int), c->stream));
        PROFILED(c, NLE_K_SMALL, nlek::plane_matches_levels(c->stream, d_x + (long long)t.row0 * t.gs.W, t.lev.p,
                                                            (long long)t.nrows * t.gs.W, d_differs.p));
    }
    {
        ProfObserver obs(c, kProfTableReduce);
        HIP_OK(nlek::sink_hist_tiled(c->stream, nlek::ROWPASS_XVEC, view, nullptr, NLE_EPS, nullptr, d_ws.p, d_m.p, &obs, d_x,
                                     d_differs.p));
    }
    all_reduce(c, d_m.p, P64);
    // x at the p sample pixels: every rank's own rows, completed by the all-reduce when the planes are slabs
    DevBuf<double> d_xA(p);
    {
        const bool slabs = c->slab_input && c->world > 1;
        PROFILED(c, NLE_K_SMALL, nlek::gather_samples_slab(c->stream, d_x, t.gs, slabs ? f->row0 : 0, slabs ? f->row1 : f->H, d_xA.p,
                                                           d_differs.p));
        if (slabs) all_reduce(c, d_xA.p, p);
    }
    PROFILED(c, NLE_K_SMALL, nlek::apply_small(c->stream, p, K, t.ldd, L, P64, d_m.p, t.D.p, t.Vrows.p, d_xA.p, d_resp.p,
                                               d_t.p, d_Wp.p, d_YA.p, d_differs.p, t.m_train.p, t.xA_train.p));
    int lb = std::min(L, nlek::apply_layers_per_launch(view));
    if (group > 0) lb = std::min(lb, group);
    DevBuf<double> d_gws((size_t)lb * t.nrows * 256 * t.gs.nSelCols);
    for (int l = 0; l < L; l += lb) {
        const int nl = std::min(lb, L - l);
        {
            ProfObserver obs(c, kProfTableExpand);
            HIP_OK(nlek::apply_hist_layers(c->stream, view, d_Wp.p + (size_t)l * P64, P64, nl, d_gws.p, d_y + (size_t)l * M, M,
                                           &obs, round8));
        }
        PROFILED(c, NLE_K_SMALL, nlek::scatter_samples(c->stream, p, nl, t.sample_loc.p, d_YA.p + (size_t)l * p,
                                                       d_y + (size_t)l * M, M, round8));
        if (done) done(l, nl);
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    prof_flush(c);
}

// The batched form.  Reduce half: the planes in groups of sorted_planes_per_launch, one pass over the sorted rows per group
// (a last group of one plane takes the single pass); the p-sized middle per plane, with that plane's responses.  Expand
// half: the R weight vectors in groups of apply_layers_per_launch, whatever plane they belong to.  Every input is read
// before the first output is written.  Workspace: one group's tables, not P or R of them.
void apply_sample_space_planes(nle_filter* f, const float* const* d_x, int P, const int* nresp, const double* h_g, int R,
                               float* d_y, long long ystride, bool round8) {
    nle_ctx* c = f->ctx;
    const TableFilter& t = *f->tables;
    const nlek::TableView view = t.view();
    const int p = t.p, K = f->K, P64 = t.P64;
    const int NP = std::min(P, nlek::sorted_planes_per_launch(t.gs));
    DevBuf<double> d_ws(nlek::apply_reduce_planes_workspace_elems(t.gs, t.nrows, NP)), d_m((size_t)NP * P64),
        d_resp((size_t)R * K), d_t(K), d_xA(p), d_Wp((size_t)R * P64), d_YA((size_t)R * p);
    HIP_OK(hipMemcpyAsync(d_resp.p, h_g, (size_t)R * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    int j = 0;  // first response of the plane in hand
    for (int m0 = 0; m0 < P; m0 += NP) {
        const int np = std::min(NP, P - m0);
        {
            ProfObserver obs(c, kProfTableReduce);
            if (np > 1) HIP_OK(nlek::apply_reduce_planes(c->stream, view, d_x + m0, np, d_ws.p, d_m.p, &obs));
            else HIP_OK(nlek::sink_hist_tiled(c->stream, nlek::ROWPASS_XVEC, view, nullptr, NLE_EPS, nullptr, d_ws.p, d_m.p, &obs, d_x[m0]));
        }
        for (int m = m0; m < m0 + np; ++m) {
            const int L = nresp[m];
            PROFILED(c, NLE_K_SMALL, nlek::gather_samples_slab(c->stream, d_x[m], t.gs, 0, f->H, d_xA.p));
            PROFILED(c, NLE_K_SMALL, nlek::apply_small(c->stream, p, K, t.ldd, L, P64, d_m.p + (size_t)(m - m0) * P64, t.D.p,
                                                       t.Vrows.p, d_xA.p, d_resp.p + (size_t)j * K, d_t.p, d_Wp.p + (size_t)j * P64,
                                                       d_YA.p + (size_t)j * p));
            j += L;
        }
    }
    const int lb = std::min(R, nlek::apply_layers_per_launch(view));
    DevBuf<double> d_gws((size_t)lb * t.nrows * 256 * t.gs.nSelCols);
    for (int l = 0; l < R; l += lb) {
        const int nl = std::min(lb, R - l);
        {
            ProfObserver obs(c, kProfTableExpand);
            HIP_OK(nlek::apply_hist_layers(c->stream, view, d_Wp.p + (size_t)l * P64, P64, nl, d_gws.p, d_y + (size_t)l * ystride,
                                           ystride, &obs, round8));
        }
        PROFILED(c, NLE_K_SMALL, nlek::scatter_samples(c->stream, p, nl, t.sample_loc.p, d_YA.p + (size_t)l * p,
                                                       d_y + (size_t)l * ystride, ystride, round8));
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    prof_flush(c);
}

// t = V^T x of P planes on a table filter (nle_filter_coefficients): the reduce half and the p-sized middle exactly as the
// two applies above run them -- one plane, or a filter without level-sorted rows: apply_sample_space's, training's own
// reduce half included where that apply takes it; several planes on sorted rows: apply_sample_space_planes' groups -- with
// one response of ones, whose W' and YA are dropped: what k_apply_small writes to t_out is the vector handed out.  world == 1.
void coefficients_sample_space(nle_filter* f, const float* const* d_x, int P, double* h_t) {
    nle_ctx* c = f->ctx;
    const TableFilter& t = *f->tables;
    const nlek::TableView view = t.view();
    const int p = t.p, K = f->K, P64 = t.P64;
    const bool batched = P > 1 && t.sorted_rows() != nullptr;
    const int NP = batched ? std::min(P, nlek::sorted_planes_per_launch(t.gs)) : 1;
    DevBuf<double> d_ws(batched ? nlek::apply_reduce_planes_workspace_elems(t.gs, t.nrows, NP)
                                : nlek::hist_tiled_workspace_elems(t.gs, t.nrows)),
        d_m((size_t)NP * P64), d_resp(K), d_t((size_t)P * K), d_xA(p), d_Wp(P64), d_YA(p);
    const std::vector<double> ones((size_t)K, 1.0);
    HIP_OK(hipMemcpyAsync(d_resp.p, ones.data(), (size_t)K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    DevBuf<int> d_differs;
    const bool reuse = !batched && t.m_train.p && !c->comm && c->train_reduce;
    if (reuse) d_differs.alloc(1);
    for (int m0 = 0; m0 < P; m0 += NP) {
        const int np = std::min(NP, P - m0);
        if (reuse) {
            HIP_OK(hipMemsetAsync(d_differs.p, 0, sizeof(int), c->stream));
            PROFILED(c, NLE_K_SMALL, nlek::plane_matches_levels(c->stream, d_x[m0] + (long long)t.row0 * t.gs.W, t.lev.p,
                                                                (long long)t.nrows * t.gs.W, d_differs.p));
        }
        {
            ProfObserver obs(c, kProfTableReduce);
            if (np > 1) HIP_OK(nlek::apply_reduce_planes(c->stream, view, d_x + m0, np, d_ws.p, d_m.p, &obs));
            else HIP_OK(nlek::sink_hist_tiled(c->stream, nlek::ROWPASS_XVEC, view, nullptr, NLE_EPS, nullptr, d_ws.p, d_m.p, &obs,
                                              d_x[m0], d_differs.p));
        }
        for (int m = m0; m < m0 + np; ++m) {
            PROFILED(c, NLE_K_SMALL, nlek::gather_samples_slab(c->stream, d_x[m], t.gs, 0, f->H, d_xA.p, d_differs.p));
            PROFILED(c, NLE_K_SMALL, nlek::apply_small(c->stream, p, K, t.ldd, 1, P64, d_m.p + (size_t)(m - m0) * P64, t.D.p,
                                                       t.Vrows.p, d_xA.p, d_resp.p, d_t.p + (size_t)m * K, d_Wp.p, d_YA.p,
                                                       d_differs.p, t.m_train.p, t.xA_train.p));
        }
    }
    HIP_OK(hipMemcpyAsync(h_t, d_t.p, (size_t)P * K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    prof_flush(c);
}

}  // namespace nlep

extern "C" int nle_filter_level_tiles(const nle_filter* f, int* first_tile, int* n_tiles) {
    if (!f || !first_tile || !n_tiles) return NLE_ERR_INVALID;
    const nlek::SortedRows* sr = f->tables ? f->tables->sorted_rows() : nullptr;
    *first_tile = sr ? sr->lev_t0 : 0;
    *n_tiles = sr ? sr->lev_nt : 16;
    return NLE_OK;
}
