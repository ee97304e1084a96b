// What crosses the host-side translation units of the train and apply orchestration: pipeline.hip (checks, dispatch, apply and
// the entry points), literal.hip (materialised Phi in fp32 and fp64), sample_space.hip (table, Phi-free and streamed fp64
// formulations) and exact_train.hip (the exact filter).  Not installed, not part of the ABI.
#pragma once
#include "ortho.h"
#include "samples.h"

namespace nlep {

// The image and sample-grid checks of every entry point that takes a plane and sample counts
GridSpec checked_grid(int H, int W, int nRow, int nCol);
// (c null: everything on the host; the switches come as an argument either way)
Nystrom solve_Ka(nle_ctx* c, const nlesw::Switches& sw, const std::vector<double>& Ka, int p, bool allow_chol);
// Exact sample rows: row a of the column-major host matrix src (nrows x K) is written, zero padded to ld, over the row of
// sample a's pixel in the device matrix d_X (this rank's slab [pix0, pix0 + M), ld columns); samples of other slabs are
// skipped.  Returns with the stream drained (the host staging vectors go out of scope).
template <typename T>
void scatter_sample_rows(nle_ctx* c, const std::vector<long long>& pix, int nrows, const std::vector<double>& src, int K,
                         int ld, long long pix0, long long M, T* d_X) {
    std::vector<T> rows;
    std::vector<long long> idx;
    for (int a = 0; a < nrows; ++a) {
        const long long loc = pix[a] - pix0;
        if (loc < 0 || loc >= M) continue;
        idx.push_back(loc);
        const size_t off = rows.size();
        rows.resize(off + ld, T(0));
        for (int k = 0; k < K; ++k) rows[off + k] = (T)src[(size_t)k * nrows + a];
    }
    DevBuf<T> d_rows(rows.size());
    DevBuf<long long> d_idx(idx.size());
    if (!idx.empty()) {
        HIP_OK(hipMemcpyAsync(d_rows.p, rows.data(), rows.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(d_idx.p, idx.data(), idx.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
        if constexpr (std::is_same<T, float>::value)
            PROFILED(c, NLE_K_SMALL, nlek::scatter_rows(c->stream, d_rows.p, d_idx.p, (int)idx.size(), ld, d_X, M));
        else
            PROFILED(c, NLE_K_SMALL, nlek::scatter_rows64(c->stream, d_rows.p, d_idx.p, (int)idx.size(), ld, d_X, M));
    }
    HIP_OK(hipStreamSynchronize(c->stream));
}

// what the filter keeps of the orthogonalisation (O: Ortho or OrthoSS) and of solve_Ka
template <typename O>
void adopt_ortho(nle_filter* f, const O& o) {
    f->K = o.K, f->ldv = ld4(o.K), f->eigvals = o.Sq;
    f->r_wa = o.r_wa, f->r_q = o.r_q, f->chol_wa = o.chol_wa ? 1 : 0;
}
inline void adopt_nystrom(nle_filter* f, const Nystrom& ny, int formulation) {
    f->r = ny.r, f->chol_ka = ny.chol ? 1 : 0, f->formulation = formulation;
}

// Head and tail that train_impl and train_exact_impl share.  begin_train: the new filter with this rank's rows, the call's clock
// started, the page-locked staging block reset.  end_train (the stream is drained): profile records, ms[5], registration.
std::unique_ptr<nle_filter> begin_train(nle_ctx* c, int H, int W, double* t_begin);
nle_filter* end_train(std::unique_ptr<nle_filter> f, double t_begin);

// The fp64 pass takes the logical width: it never loads a column >= r (nle.h: "leading dimension any value >= the logical
// width"), and its vectors have ld4(r) entries.  The fp32 pass reads whole rows of ld (a multiple of 4, padding zero).
template <typename T>
hipError_t rowpass_any(hipStream_t s, int mode, const T* X, long long M, int ld, int r, const double* t, const double* lam,
                       const float* xv, double eps, double* partial, int* nb) {
    if constexpr (std::is_same<T, float>::value) return nlek::rowpass(s, mode, X, M, ld, t, lam, xv, eps, partial, nb);
    else return nlek::rowpass64(s, mode, X, M, ld, r, t, lam, xv, eps, partial, nb);
}
template <typename T>  // (the fp64 kernel takes K)
hipError_t apply_expand_any(hipStream_t s, const T* V, long long M, int ld, int K, const double* g, int L, float* Y,
                            long long ldy) {
    if constexpr (std::is_same<T, float>::value) return nlek::apply_expand(s, V, M, ld, g, L, Y, ldy);
    else return nlek::apply_expand64(s, V, M, ld, K, g, L, Y, ldy);
}

// unpack the upper-triangular ts x ts tile list of gram() / gram64() into a symmetric n x n matrix (literal.hip)
std::vector<double> unpack_tiles(const std::vector<double>& tiles, int ld, int n, int ts);

// One train call's arguments and stage clocks; the path train_impl chooses fills f->K, ldv, eigvals and V or V64 (or f->tables)
using SolveKa = std::function<Nystrom()>;
struct TrainPath {
    nle_ctx* c;
    nle_filter* f;
    const float* d_lum;
    const SampleSet& ss;
    double hx, hy;
    int T, n_eig;
    long long pix0, M;  // this rank's pixels
    double* host_ms;  // host-side milliseconds of the call
    Trace& tr;
    Timer tm_s{c->stream}, tm_g{c->stream}, tm_p{c->stream};  // Sinkhorn, Gram, projection
    void train_materialised(const Nystrom& ny);  // literal.hip
    void train_generic64(const Nystrom& ny);
    void train_tables(const SolveKa& solve);  // sample_space.hip
    void train_phi_free_exp(const SolveKa& solve);
    void train_stream64(const SolveKa& solve);
};

// X (p x K column-major on the host) as the p x ldd row-major, zero-padded operand of project64 (sample_space.hip)
std::vector<double> padded_rows(const std::vector<double>& X, int p, int K, int ldd);
std::vector<double> host_Vrows(const nle_filter* f);  // sample_space.hip, as the next two
void ensure_V(nle_filter* f);
// `done(l0, nl)`, when given, is called after layers [l0, l0 + nl) are complete on the stream (the host-buffer entry
// points start their download there); `group` caps the layers per launch (0: as many as fit)
using LayersDone = std::function<void(int, int)>;
// ystride: floats between the output layers (0: n_local, the layer-major block nle_apply_layers writes)
void apply_sample_space(nle_filter* f, const float* d_x, const double* h_g /* L x K */, int L, float* d_y,
                        const LayersDone& done = nullptr, int group = 0, bool round8 = false, long long ystride = 0);
// The same for P planes at once on a table filter with level-sorted rows, world == 1: plane m is
// d_x[m] with nresp[m] responses, h_g the R = sum nresp rows of K (plane 0's first), output j at d_y + j * ystride.  The
// reduce half walks the sorted rows once per group of nlek::sorted_planes_per_launch planes; every output is bit for bit
// what apply_sample_space writes for its plane alone.
void apply_sample_space_planes(nle_filter* f, const float* const* d_x, int P, const int* nresp, const double* h_g, int R,
                               float* d_y, long long ystride, bool round8);
// t = V^T x of P planes on a table filter, world == 1: h_t P x K, row m the bits the applies above form for plane m
// (nle_filter_coefficients)
void coefficients_sample_space(nle_filter* f, const float* const* d_x, int P, double* h_t);
// exact_train.hip
nle_filter* train_exact_impl(nle_ctx* c, const float* d_lum, int H, int W, double hx, double hy, int T, int n_eig);

}  // namespace nlep
