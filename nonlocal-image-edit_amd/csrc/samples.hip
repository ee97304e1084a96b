// The sample set and the fp64 affinity rows on the host: see samples.h.
#include "samples.h"

namespace nlep {

namespace {
template <typename T>
T* upload(hipStream_t st, DevBuf<T>& d, const std::vector<T>& h) {  // enqueued: h must outlive the copy
    d.alloc(h.size());
    HIP_OK(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return d.p;
}

// the integer sum of squared differences of rows i and j of v (d values per row)
long long ssd(const std::vector<int>& v, int d, int i, int j) {
    const int *vi = v.data() + (size_t)i * d, *vj = v.data() + (size_t)j * d;
    long long S = 0;
    for (int k = 0; k < d; ++k) S += (long long)(vi[k] - vj[k]) * (vi[k] - vj[k]);
    return S;
}

// One B operand of the patch kernels and its norms, on the host: row j = the d values of sample j in each of `planes`, one
// plane after the other, shifted by -128 as int8 and zero padded to kp bytes (rows p .. roundup16(p) zero: `total` bytes
// in all); norm[j] = the sum of the squares of those int8 values
struct PackedInt8 {
    std::vector<signed char> bytes;
    std::vector<int> norm;
};
PackedInt8 pack_int8(std::initializer_list<const std::vector<int>*> planes, int p, int d, int kp, size_t total) {
    PackedInt8 o{std::vector<signed char>(total, 0), std::vector<int>(p, 0)};
    for (int j = 0; j < p; ++j) {
        int k = 0;
        for (const std::vector<int>* plane : planes)
            for (int q = 0; q < d; ++q, ++k) {
                const int v = (*plane)[(size_t)j * d + q] - 128;
                o.bytes[(size_t)j * kp + k] = (signed char)v;
                o.norm[j] += v * v;
            }
    }
    return o;
}
}  // namespace

AffinityOpts affinity_opts(const nle_ctx* c) {
    AffinityOpts o;
    o.R = c->patch_radius;
    o.d_a = c->chroma_a;  // nle_ctx_set_chroma sets both planes and hc > 0, or neither and 0
    o.d_b = c->chroma_b;
    o.hc = c->chroma_hc;
    o.sampler = c->sampler;
    return o;
}

void check_affinity_opts(const nle_ctx* c, const AffinityOpts& o, const GridSpec& gs, int H, int W, double hx, double hy,
                         Caller where) {
    if (where == Caller::KERNEL32 || where == Caller::NYSTROM32) {  // the fp32 stages take none of the options
        const std::string who = where == Caller::KERNEL32 ? "nle_compute_kernel (fp32) " : "nle_nystrom (fp32) ";
        const std::string use = where == Caller::KERNEL32 ? ": use nle_compute_kernel64" : ": use the fp64 formulations";
        if (o.patch()) throw Fail{NLE_ERR_INVALID, who + "does not take patch affinities" + use};
        if (o.chroma()) throw Fail{NLE_ERR_INVALID, who + "does not take chroma affinities" + use};
        if (o.listed()) throw Fail{NLE_ERR_INVALID, who + "takes the grid sampler only" + use};
        return;
    }
    // train: the fp64 formulations with explicit affinity rows only -- the table form needs single values of a Cartesian
    // set (a 256-level table cannot index a patch or a colour triple), the other forms are fp32
    const bool mode_ok = where != Caller::TRAIN || c->mode == NLE_MODE_AUTO || c->mode == NLE_MODE_MATERIALISED_F64 ||
                         c->mode == NLE_MODE_STREAMED_F64;
    auto check_mode = [&](const std::string& what, bool plural) {
        if (!mode_ok)
            throw Fail{NLE_ERR_INVALID, what + (plural ? " run" : " runs") + " in NLE_MODE_AUTO, NLE_MODE_MATERIALISED_F64 or "
                                        "NLE_MODE_STREAMED_F64 only"};
    };
    // the patches, the chroma planes and the sampler's selection all reach over the whole image
    auto check_slab = [&](const std::string& what, bool plural) {
        if (c->slab_input && c->world > 1)
            throw Fail{NLE_ERR_INVALID, what + (plural ? " need" : " needs") + " the full plane on every rank: slab input is "
                                        "not supported with " + (plural ? "them" : "it")};
    };
    if (o.patch() && where != Caller::SAMPLE_PIXELS) {  // nle_ctx_set_patch_radius has checked 0 <= R <= 7
        check_mode("patch affinities (patch radius > 0)", true);
        if (o.R > std::min(H, W) - 1)
            throw Fail{NLE_ERR_INVALID, "patch radius " + std::to_string(o.R) + " needs an image of at least " +
                                            std::to_string(o.R + 1) + " x " + std::to_string(o.R + 1) +
                                            " pixels (R <= min(H, W) - 1)"};
        check_slab("patch affinities (patch radius > 0)", true);
    }
    if (o.chroma() && where != Caller::SAMPLE_PIXELS) {
        if (where == Caller::KERNEL64 && !(hx > 0 && hy > 0)) throw Fail{NLE_ERR_INVALID, "hx and hy must be > 0"};
        check_mode("chroma affinities (nle_ctx_set_chroma)", true);
        if (o.R > NLE_CHROMA_PATCH_RADIUS_MAX)
            throw Fail{NLE_ERR_INVALID, "chroma affinities take a patch radius of at most " +
                                            std::to_string(NLE_CHROMA_PATCH_RADIUS_MAX) + ", got " + std::to_string(o.R)};
        check_slab("chroma affinities", true);
        // the samples' tables of the affinity kernels live in LDS
        const int p = gs.p(), ld = ld4(p);
        const bool fits = o.patch() ? nlek::patch_affinity64_chroma_lds_bytes(ld) <= nlek::kPatchChromaLdsMax
                                    : nlek::affinity64_chroma_lds_bytes(ld) <= nlek::kDynLdsDefault;
        if (!fits)
            throw Fail{NLE_ERR_INVALID, "chroma affinities: " + std::to_string(p) + " samples do not fit the affinity kernel's "
                                        "LDS tables (at most 2728 at patch radius 0, 5984 above)"};
    }
    if (o.listed()) {
        check_mode(o.sampler_name(), false);
        if (!(hx > 0) || !(hy > 0)) throw Fail{NLE_ERR_INVALID, "hx and hy must be > 0"};
        check_slab(o.sampler_name(), false);
        if (o.sampler == NLE_SAMPLER_RESIDUAL && gs.p() > nlek::kResidMaxSamples)
            throw Fail{NLE_ERR_INVALID, "the residual sampler takes at most 2048 samples, got " + std::to_string(gs.p())};
    }
}

SampleSet fetch_samples(nle_ctx* c, const float* d_lum, const GridSpec& gs, const AffinityOpts& o, const FetchSpec& spec) {
    SampleSet s;
    s.gs = gs;
    s.p = gs.p();
    s.opts = o;
    const std::vector<long long>* list = spec.list;
    const bool check_quantised = spec.check_levels || o.patch() || o.chroma();
    if ((list != nullptr) != o.listed() || (list && ((int)list->size() != s.p || spec.slab_plane)))
        throw Fail{NLE_ERR_INVALID, "fetch_samples: bad sample list"};
    if (o.chroma() && spec.slab_plane) throw Fail{NLE_ERR_INVALID, "fetch_samples: no chroma planes"};
    s.val.resize(s.p);
    const bool slabs = spec.slab_plane;
    int row0 = 0, row1 = gs.H;  // the rows that exist behind d_lum
    if (slabs) slab(gs.H, c->rank, c->world, &row0, &row1);
    int fl2[2] = {1, 0xffff};  // check_levels: [0] != 0: not integer valued, [1] level tiles
    DevBuf<double> d_v(slabs ? (size_t)s.p + 1 : 0);  // slabs: the values (0 outside these rows) + the verdict, summed over ranks
    DevBuf<float> d_val(slabs ? 0 : (size_t)s.p);
    DevBuf<int> d_flag(2);
    DevBuf<long long> d_pix;
    if (slabs) {
        PROFILED(c, NLE_K_SMALL, nlek::gather_samples_slab(c->stream, d_lum, gs, row0, row1, d_v.p));
    } else if (list) {
        PROFILED(c, NLE_K_SMALL, nlek::gather_pix(c->stream, d_lum, upload(c->stream, d_pix, *list), s.p, d_val.p));
    } else {
        PROFILED(c, NLE_K_SMALL, nlek::gather_samples(c->stream, d_lum, gs, d_val.p));
    }
    if (check_quantised) {
        PROFILED(c, NLE_K_SMALL, nlek::check_levels(c->stream, d_lum + (size_t)row0 * gs.W, (long long)(row1 - row0) * gs.W, d_flag.p));
        HIP_OK(hipMemcpyAsync(fl2, d_flag.p, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    if (!slabs) HIP_OK(hipMemcpyAsync(s.val.data(), d_val.p, s.p * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (!slabs || check_quantised) HIP_OK(hipStreamSynchronize(c->stream));
    bool not_integer = !check_quantised || fl2[0] != 0;
    if (slabs) {
        const double fl = not_integer ? 1.0 : 0.0;
        std::vector<double> v((size_t)s.p + 1);
        HIP_OK(hipMemcpyAsync(d_v.p + s.p, &fl, sizeof(double), hipMemcpyHostToDevice, c->stream));
        all_reduce(c, d_v.p, v.size());
        HIP_OK(hipMemcpyAsync(v.data(), d_v.p, v.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        for (int k = 0; k < s.p; ++k) s.val[k] = (float)v[k];
        not_integer = v[s.p] > 0.0;
    }
    s.quantised = !not_integer;
    if (s.quantised && (fl2[1] & 0xffff) != 0) s.level_tiles = (unsigned)fl2[1] & 0xffffu;
    s.pix.resize(s.p);
    s.packed.resize(s.p);
    for (int k = 0; k < s.p; ++k) {
        const int r = list ? (int)((*list)[k] / gs.W) : gs.rowOff + (k / gs.nSelCols) * gs.rowStep;
        const int cc = list ? (int)((*list)[k] - (long long)r * gs.W) : gs.colOff + (k % gs.nSelCols) * gs.colStep;
        s.pix[k] = (long long)r * gs.W + cc;
        s.packed[k] = make_float4((float)r, (float)cc, s.val[k], 0.f);
    }
    if (!o.patch() && !o.chroma()) return s;
    // the (2R + 1)^2 values around every sample of the L plane (R > 0) and of the a and b planes (chroma; R = 0: the one-value
    // patch is the pixel itself), and the level check of a and b: enqueued together, one synchronisation
    const size_t n = (size_t)s.p * o.patch_len();
    DevBuf<int> d_patch(((o.patch() ? 1 : 0) + (o.chroma() ? 2 : 0)) * n), d_flag4(4);
    int fl4[4] = {1, 0, 1, 0}, nplanes = 0;
    if (!list) upload(c->stream, d_pix, s.pix);  // (a list is there already)
    auto gather = [&](const float* d_plane, std::vector<int>* out) {  // enqueues; *out is complete after the synchronisation
        int* d_out = d_patch.p + (size_t)nplanes++ * n;
        out->resize(n);
        PROFILED(c, NLE_K_SMALL, nlek::patch_gather(c->stream, d_plane, gs.H, gs.W, o.R, d_pix.p, s.p, d_out));
        HIP_OK(hipMemcpyAsync(out->data(), d_out, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    };
    if (o.patch()) gather(d_lum, &s.patch);
    if (o.chroma()) {
        gather(o.d_a, &s.aval);
        gather(o.d_b, &s.bval);
        PROFILED(c, NLE_K_SMALL, nlek::check_levels(c->stream, o.d_a, (long long)gs.H * gs.W, d_flag4.p));
        PROFILED(c, NLE_K_SMALL, nlek::check_levels(c->stream, o.d_b, (long long)gs.H * gs.W, d_flag4.p + 2));
        HIP_OK(hipMemcpyAsync(fl4, d_flag4.p, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    s.chroma_quantised = o.chroma() && fl4[0] == 0 && fl4[2] == 0;
    return s;
}

namespace {
// NLE_SAMPLER_FARTHEST on this rank: the samples in the order chosen, into v[0 .. p)
void farthest_select(nle_ctx* c, const float* d_lum, const GridSpec& gs, double hx, double hy, double* v) {
    const int p = gs.p(), nb = nlek::farthest_max_blocks();
    DevBuf<double> d_m((size_t)gs.H * gs.W), d_pv((size_t)2 * nb);
    DevBuf<int> d_pi((size_t)2 * nb), d_list(p);
    std::vector<int> idx(p);
    PROFILED(c, NLE_K_SMALL, nlek::farthest_samples(c->stream, d_lum, gs.H, gs.W, p, 1.0 / (hx * hx), 1.0 / (hy * hy), d_m.p,
                                                    d_pv.p, d_pi.p, d_list.p));
    HIP_OK(hipMemcpyAsync(idx.data(), d_list.p, p * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < p; ++k) v[k] = (double)idx[k];
}

// NLE_SAMPLER_RESIDUAL on this rank; `order`: also pivots, n_residual and the statistics of the whole set (one more round)
void residual_select(nle_ctx* c, const float* d_lum, const GridSpec& gs, double hx, double hy, double* v, SamplerOrder* order) {
    const int p = gs.p(), nb = nlek::farthest_max_blocks();
    const size_t N = (size_t)gs.H * gs.W, ld = (size_t)nlek::residual_ld((long long)N);
    // the factor is the one large buffer: refused before anything is enqueued if it cannot fit (what the cache holds counts
    // as free: arena_alloc drops it when hipMalloc fails)
    const size_t need = ld * p * sizeof(double);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b + c->arena_bytes)
        throw Fail{NLE_ERR_INVALID, "the residual sampler holds its factor in device memory: " + std::to_string(need) +
                                        " bytes needed (nle_residual_sampler_bytes), " +
                                        std::to_string(free_b + c->arena_bytes) + " free"};
    DevBuf<double> d_L(ld * p), d_d(N), d_m(N), d_pv((size_t)6 * nb), d_state(2 * nlek::kResidHead), d_pivot(p);
    DevBuf<int> d_pi((size_t)4 * nb), d_list(p);
    std::vector<int> idx(p);
    double state[nlek::kResidHead];
    const double* d_final = nullptr;
    PROFILED(c, NLE_K_SMALL, nlek::residual_samples(c->stream, d_lum, gs.H, gs.W, p, 1.0 / (hx * hx), 1.0 / (hy * hy), NLE_EPS,
                                                    order != nullptr, d_L.p, d_d.p, d_m.p, d_pv.p, d_pi.p, d_state.p, d_list.p,
                                                    d_pivot.p, &d_final));
    HIP_OK(hipMemcpyAsync(idx.data(), d_list.p, p * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(state, d_final, sizeof state, hipMemcpyDeviceToHost, c->stream));
    if (order) {
        order->pivot.resize(p);
        HIP_OK(hipMemcpyAsync(order->pivot.data(), d_pivot.p, p * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < p; ++k) v[k] = (double)idx[k];
    if (order) {
        order->order.assign(idx.begin(), idx.end());
        order->n_residual = (int)state[1];
        std::copy(state + 2, state + 5, order->stats);
    }
}
}  // namespace

// At world > 1 rank 0 selects and the others receive the set through the fp64 all-reduce (they add zeros; indices < 2^31
// are exact in fp64); the last slot carries rank 0's failure, so that every rank returns the same verdict.
std::vector<long long> sampler_list(nle_ctx* c, const float* d_lum, const GridSpec& gs, double hx, double hy,
                                    SamplerOrder* order) {
    const int p = gs.p();
    const AffinityOpts o = affinity_opts(c);
    std::vector<long long> list(p);
    std::vector<double> v((size_t)p + 1, 0.0);
    if (c->rank == 0 || c->world <= 1) {
        try {
            if (o.sampler == NLE_SAMPLER_RESIDUAL) residual_select(c, d_lum, gs, hx, hy, v.data(), order);
            else farthest_select(c, d_lum, gs, hx, hy, v.data());
        } catch (const Fail&) {
            if (c->world <= 1) throw;
            v[p] = 1.0;
        }
    }
    if (c->world > 1) {
        DevBuf<double> d_v((size_t)p + 1);
        HIP_OK(hipMemcpyAsync(d_v.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        all_reduce(c, d_v.p, (size_t)p + 1);
        HIP_OK(hipMemcpyAsync(v.data(), d_v.p, v.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        if (v[p] != 0.0) throw Fail{NLE_ERR_HIP, std::string(o.sampler_name()) + " failed on rank 0"};
    }
    for (int k = 0; k < p; ++k) list[k] = (long long)v[k];
    std::sort(list.begin(), list.end());
    return list;
}

void require_integer_planes(nle_ctx* c, const SampleSet& ss, bool agree_over_ranks) {
    auto refused = [&](bool here) { return agree_over_ranks ? ranks_where(c, here) > 0 : here; };
    if (ss.opts.patch() && refused(!ss.quantised))
        throw Fail{NLE_ERR_INVALID, "patch affinities (patch radius > 0) need an integer-valued luminance plane in [0, 255] "
                                    "(the L channel of 8-bit Lab)"};
    if (ss.opts.chroma() && refused(!ss.quantised || !ss.chroma_quantised))
        throw Fail{NLE_ERR_INVALID, "chroma affinities need integer-valued L, a and b planes in [0, 255] (the channels of "
                                    "8-bit Lab)"};
}

// The exponent is -sw d2 - (intensity term), then - cwd S_ab with chroma, every operation rounded on its own: the order of
// k_affinity64 and k_patch_affinity64.  Intensity term: pw dv^2 on the fp32 values (R = 0), pwd S on the integer patches
// (R > 0: S in exact integer arithmetic).
std::vector<double> build_Ka(const SampleSet& s, double hx, double hy) {
    const int p = s.p, d = s.opts.patch_len();
    const bool patch = s.opts.patch(), chroma = s.opts.chroma();
    const double sw = 1.0 / (hx * hx), pw = 1.0 / (hy * hy), pwd = (1.0 / (hy * hy)) / d;
    const double cwd = chroma ? s.opts.cwd() : 0.0;
    std::vector<double> Ka((size_t)p * p);
    auto column = [&](int j) {
        const int rj = (int)(s.pix[j] / s.gs.W), cj = (int)(s.pix[j] % s.gs.W);
        for (int i = j; i < p; ++i) {
            const int ri = (int)(s.pix[i] / s.gs.W), ci = (int)(s.pix[i] % s.gs.W);
            const long long dr = ri - rj, dc = ci - cj;
            const double sq = (double)(dr * dr + dc * dc);
            const double dv = (double)s.val[i] - (double)s.val[j];
            const double intensity = patch ? pwd * (double)ssd(s.patch, d, i, j) : pw * (dv * dv);
            double e = -sw * sq - intensity;
            // subtracted last (include/nle.h); S_ab: the squared differences of the a and of the b values
            if (chroma) e = e - cwd * (double)(ssd(s.aval, d, i, j) + ssd(s.bval, d, i, j));
            const double v = std::exp(e);
            Ka[(size_t)j * p + i] = v;
            Ka[(size_t)i * p + j] = v;
        }
    };
    // p (p + 1) / 2 libm exponentials: 1.5 ms on one core at p = 900, before anything else of the train can start.  From
    // 384 samples on, 8 short-lived threads take BLOCKS of columns of equal triangle area (same values: every entry has one
    // writer; dealing the columns round-robin had the threads' mirrored writes share every cache line: 6.7 ms)
    const int nt = p >= 384 ? 8 : 1;
    std::vector<int> cut(nt + 1, p);
    for (int t = 0; t < nt; ++t) cut[t] = (int)(p * (1.0 - std::sqrt(1.0 - (double)t / nt)));
    nleh::run_parts(nt, nt, [&](int t) {
        for (int j = cut[t]; j < cut[t + 1]; ++j) column(j);
    });
    return Ka;
}

DevBuf<float4> upload_samples(nle_ctx* c, const SampleSet& ss, int padded) {
    DevBuf<float4> d((size_t)std::max(ss.p, padded));
    if (padded > ss.p) HIP_OK(hipMemsetAsync(d.p, 0, d.n * sizeof(float4), c->stream));
    HIP_OK(hipMemcpyAsync(d.p, ss.packed.data(), ss.p * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    return d;
}

AffinityRows64::AffinityRows64(nle_ctx* c, const float* d_lum, const SampleSet& ss, double hx, double hy, bool want_mask)
    : st_(c->stream), samples_(upload_samples(c, ss)) {
    const AffinityOpts& o = ss.opts;
    const int p = ss.p, d = o.patch_len();
    nlek::Affinity64Args& a = args_;  // the operands that are not made below stay null
    a.lum = d_lum;
    a.gs = ss.gs;
    a.samples = samples_.p;
    a.p = p;
    a.ld = ld4(p);
    a.sw = 1.0 / (hx * hx);
    a.pw = o.patch() ? (1.0 / (hy * hy)) / d : 1.0 / (hy * hy);  // R > 0: pwd, the weight of the patch sum S
    a.R = o.R;
    a.a = o.d_a;
    a.b = o.d_b;
    a.cw = o.chroma() ? o.cwd() : 0.0;
    PackedInt8 h_l, h_ab;  // host staging: alive until the stream is drained below
    std::vector<float2> h_sab;
    DevBuf<long long> d_spix;
    if (o.patch()) {
        h_l = pack_int8({&ss.patch}, p, d, nlek::patch_kpad(o.R), nlek::patch_spatch_bytes(p, o.R));
        a.spatch = upload(st_, spatch_, h_l.bytes);
        a.snorm = upload(st_, snorm_, h_l.norm);
    }
    if (o.chroma() && o.patch()) {
        h_ab = pack_int8({&ss.aval, &ss.bval}, p, d, nlek::patch_ckpad(o.R), nlek::patch_cpatch_bytes(p, o.R));
        a.cpatch = upload(st_, cpatch_, h_ab.bytes);
        a.cnorm = upload(st_, cnorm_, h_ab.norm);
    } else if (o.chroma()) {
        h_sab.resize(p);
        for (int j = 0; j < p; ++j) h_sab[j] = make_float2((float)ss.aval[j], (float)ss.bval[j]);
        a.sab = upload(st_, sab_, h_sab);
    }
    if (want_mask && o.listed()) {  // a listed sample set: its rows are zeroed by bitmask instead of the grid's closed form
        const long long N = (long long)ss.gs.H * ss.gs.W;
        mask_.alloc((size_t)((N + 31) / 32));
        PROFILED(c, NLE_K_SMALL, nlek::sample_mask(st_, upload(st_, d_spix, ss.pix), p, N, mask_.p));
        a.smask = mask_.p;
    }
    if (o.patch() || o.chroma() || a.smask) HIP_OK(hipStreamSynchronize(st_));  // the staging buffers go out of scope
}

}  // namespace nlep
