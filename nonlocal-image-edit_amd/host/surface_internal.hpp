// What the translation units of the C++ surface (stages.cpp, colour.cpp, device_group.cpp, filter.cpp) share, and the
// one owner of every step NLEFilter repeats: the process's shared ctx and its mode, status -> exception, the RAII device
// buffer, the plane conversions, the options a train sets on a ctx (TrainOptions), the colour prologue (lab_planes) and
// epilogue (lab_to_rows), their deep-colour forms (lab16_planes, lab16_to_image) and their tone-mapping forms (hdr_planes,
// hdr_to_image).  Not installed: include/nle/filter.hpp is the surface.
#pragma once

#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "nle.h"
#include "nle/filter.hpp"

namespace nle::surface {

// the mode a ctx of this process is created with (NLE_MODE, default auto): what a train with NLEFilter::exact restores
inline int default_mode() {
    const char* m = std::getenv("NLE_MODE");
    return m ? std::atoi(m) : NLE_MODE_AUTO;
}

// one context per process, created on first use (the reference keeps no global state; this one
// only holds the HIP stream)
inline nle_ctx* shared_ctx() {
    static nle_ctx* ctx = nullptr;
    if (!ctx) {
        int dev = 0;
        if (const char* e = std::getenv("NLE_DEVICE")) dev = std::atoi(e);
        if (nle_ctx_create(dev, nullptr, &ctx) != NLE_OK)
            throw std::runtime_error(std::string("nle: cannot create GPU context: ") + nle_last_error(nullptr));
        nle_ctx_set_mode(ctx, default_mode());
    }
    return ctx;
}

inline void check(int status, nle_ctx* ctx) {
    if (status != NLE_OK) throw std::runtime_error(nle_last_error(ctx));
}

// RAII device buffer through the ABI helpers (empty until one is moved in when default-constructed)
struct Dev {
    nle_ctx* c = nullptr;
    void* p = nullptr;
    Dev() = default;
    Dev(nle_ctx* ctx, size_t bytes) : c(ctx) { check(nle_dev_alloc(c, bytes, &p), c); }
    ~Dev() {
        if (p) nle_dev_free(c, p);
    }
    Dev(Dev&& o) noexcept : c(o.c), p(o.p) { o.p = nullptr; }
    Dev& operator=(Dev&& o) noexcept {
        std::swap(c, o.c);
        std::swap(p, o.p);
        return *this;
    }
    float* f() const { return static_cast<float*>(p); }
    double* d() const { return static_cast<double*>(p); }
    unsigned char* u8() const { return static_cast<unsigned char*>(p); }
};

inline double recip0(double v, double eps = EPS) { return std::fabs(v) >= eps ? 1.0 / v : 0.0; }  // :42-54

// ---- plane conversions ----
inline std::vector<float> plane_f32(const Image& m) {
    if (m.channels() != 1 || m.depth() != NLE_64F) throw std::runtime_error("expected a 1-channel CV_64F matrix");
    std::vector<float> v(m.total());
    const double* s = m.ptr<double>();
    for (size_t i = 0; i < v.size(); ++i) v[i] = (float)s[i];
    return v;
}

// a 1-channel CV_64F plane as fp32 on the device
inline Dev upload_plane(nle_ctx* c, const Image& m) {
    const std::vector<float> v = plane_f32(m);
    Dev d(c, v.size() * 4);
    check(nle_dev_upload(c, d.p, v.data(), v.size() * 4), c);
    return d;
}

// rows x cols fp32 values as a CV_64F image
inline Image image_f64(const float* v, int rows, int cols) {
    Image m(rows, cols, NLE_64F, 1);
    double* d = m.ptr<double>();
    for (size_t i = 0; i < m.total(); ++i) d[i] = v[i];
    return m;
}

// rows of a column-major p x n fp64 matrix's TRANSPOSE, one row per pixel (n x ld), i.e. the reference's `Kab` /
// `Wab` seen as one row per pixel (the stage-level API runs on fp64 device matrices: nle_*64)
inline std::vector<double> cols_as_rows_f64(const Mat& m, int ld) {
    std::vector<double> v((size_t)m.cols() * ld, 0.0);
    for (int j = 0; j < m.cols(); ++j)
        for (int i = 0; i < m.rows(); ++i) v[(size_t)j * ld + i] = m(i, j);
    return v;
}

// ---- the options a train (or a residual map) sets on a ctx, for the length of one call ----
// Sets, in this order, the filter's patch radius, sampler, the exact mode and (with planes) chroma; puts back radius 0,
// the grid sampler, the process's mode and chroma off when the scope ends, however it ends -- also when one of its own
// setters refuses.  A ctx is shared (the free functions run on shared_ctx()), so nothing else may set these options.
// The exception of a failure inside the scope is built before the options go back: its text is the first failure's.
class TrainOptions {
public:
    TrainOptions(nle_ctx* c, const NLEFilter& f, const float* d_a, const float* d_b) : c_(c), exact_(f.exact) {
        int st = nle_ctx_set_patch_radius(c_, f.patchRadius);
        if (st == NLE_OK) st = nle_ctx_set_sampler(c_, f.sampler);
        if (st == NLE_OK && exact_) st = nle_ctx_set_mode(c_, NLE_MODE_EXACT_F64);
        if (st == NLE_OK && (d_a || d_b)) st = nle_ctx_set_chroma(c_, d_a, d_b, f.chromaBandwidth);
        if (st != NLE_OK) {
            const std::runtime_error refused(nle_last_error(c_));
            restore();
            throw refused;
        }
    }
    ~TrainOptions() { restore(); }

private:
    void restore() {
        nle_ctx_set_chroma(c_, nullptr, nullptr, 0.0);  // the planes were borrowed for this call only
        nle_ctx_set_patch_radius(c_, 0);  // the ctx's other users (the free functions) keep the reference's affinity
        nle_ctx_set_sampler(c_, NLE_SAMPLER_GRID);          // and its grid
        if (exact_) nle_ctx_set_mode(c_, default_mode());   // and its mode
    }
    nle_ctx* c_;
    bool exact_;
};

// ---- colour prologue: n BGR pixels (a whole image, or a rank's rows) -> Lab on the device ----
// bgr and L (fp32) always; lab (the 8-bit Lab image) and a, b (fp32) when wanted, empty otherwise
struct LabPlanes {
    Dev bgr, lab, L, a, b;
};
inline LabPlanes lab_planes(nle_ctx* c, const unsigned char* bgr, size_t n, bool want_lab, bool want_ab) {
    LabPlanes o;
    o.bgr = Dev(c, n * 3);
    o.L = Dev(c, n * 4);
    if (want_lab || want_ab) o.lab = Dev(c, n * 3);
    check(nle_dev_upload(c, o.bgr.p, bgr, n * 3), c);
    check(nle_bgr2lab8(c, o.bgr.u8(), (long long)n, o.lab.u8(), o.L.f()), c);
    if (want_ab) {
        o.a = Dev(c, n * 4);
        o.b = Dev(c, n * 4);
        check(nle_lab8_channel(c, o.lab.u8(), (long long)n, 1, o.a.f()), c);
        check(nle_lab8_channel(c, o.lab.u8(), (long long)n, 2, o.b.f()), c);
    }
    return o;
}

// ---- colour epilogue: Lab -> BGR into rows [r0, r1) of `out` ----
// in.lab with its L plane replaced by d_L (clamped and rounded to 8 bit) and, where given, a and b by d_a and d_b
inline void lab_to_rows(nle_ctx* c, const LabPlanes& in, const float* d_L, const float* d_a, const float* d_b, Image& out,
                        int r0, int r1) {
    const size_t n = (size_t)(r1 - r0) * out.cols;
    if (d_a || d_b) check(nle_lab2bgr8_planes(c, in.lab.u8(), d_L, d_a, d_b, (long long)n, in.bgr.u8()), c);
    else check(nle_lab2bgr8(c, in.lab.u8(), d_L, (long long)n, in.bgr.u8()), c);
    check(nle_dev_download(c, out.ptr<unsigned char>(r0), in.bgr.p, n * 3), c);
}

// ---- the pre-filter of the denoise flow (DenoiseOptions): one owner for train and denoise ----
// what a non-default DenoiseOptions may hold; sigmaColor / sigmaSpace are checked as nle_bilateral8 checks them, also when
// the NLM pre-filter leaves them unused
inline void check_denoise_options(const DenoiseOptions& o, int sigmaColor, int sigmaSpace) {
    if (o.prefilter != NLE_PREFILTER_BILATERAL && o.prefilter != NLE_PREFILTER_NLM)
        throw std::runtime_error("DenoiseOptions::prefilter must be NLE_PREFILTER_BILATERAL or NLE_PREFILTER_NLM");
    if (std::isnan(o.noiseSigma) || std::isinf(o.noiseSigma))
        throw std::runtime_error("DenoiseOptions::noiseSigma must be finite (negative: estimated)");
    if (!std::isfinite(o.nlmH) || o.nlmH < 0) throw std::runtime_error("DenoiseOptions::nlmH must be finite and >= 0 (0: from the noise level)");
    int radius = 0;
    nle_bilateral_tables(sigmaColor, sigmaSpace, &radius, nullptr, nullptr);
    if (radius > 64) throw std::runtime_error("bilateral filter: sigma_space above 42 (radius > 64) is not supported");
}

// the noise level of an 8-bit plane on the device: the caller's, or Immerkaer's estimate (nle_plane_noise)
inline double plane_sigma(nle_ctx* c, const DenoiseOptions& o, const float* d_x, int H, int W) {
    if (o.noiseSigma >= 0) return o.noiseSigma;
    double sigma = 0;
    check(nle_plane_noise(c, d_x, H, W, nullptr, &sigma), c);
    return sigma;
}

// d_dst = the pre-filtered d_src (H x W levels as fp32).  Bilateral: the reference's call.  NLM: nle_nlm8 with the IPOL
// table's P, S and h for `sigma` (see DenoiseOptions); h == 0: a copy, no kernel runs
inline void prefilter_plane(nle_ctx* c, const DenoiseOptions& o, const float* d_src, int H, int W, int sigmaColor,
                            int sigmaSpace, double sigma, float* d_dst) {
    if (o.prefilter == NLE_PREFILTER_BILATERAL) return check(nle_bilateral8(c, d_src, H, W, sigmaColor, sigmaSpace, d_dst), c);
    const int P = sigma <= 15 ? 1 : sigma <= 30 ? 2 : 3, S = 10;
    const double h = o.nlmH > 0 ? o.nlmH : (sigma <= 30 ? 0.40 : 0.35) * sigma;
    if (h == 0) {
        std::vector<float> v((size_t)H * W);
        check(nle_dev_download(c, v.data(), d_src, v.size() * 4), c);
        return check(nle_dev_upload(c, d_dst, v.data(), v.size() * 4), c);
    }
    check(nle_nlm8(c, d_src, H, W, P, S, sigma, h, d_dst, nullptr), c);
}

// ---- deep colour (16UC3 images): the same two steps on float Lab planes ----
// prologue: n 16-bit BGR pixels -> L (fp32, unrounded) always; a and b (likewise) and the guide (L rounded to the 256
// levels a train takes) when wanted, empty otherwise
struct Lab16Planes {
    Dev bgr, L, a, b, guide;
};
inline Lab16Planes lab16_planes(nle_ctx* c, const Image& image, bool want_ab, bool want_guide) {
    const size_t n = image.total();
    Lab16Planes o;
    o.bgr = Dev(c, n * 6);
    o.L = Dev(c, n * 4);
    if (want_ab) o.a = Dev(c, n * 4);
    if (want_ab) o.b = Dev(c, n * 4);
    if (want_guide) o.guide = Dev(c, n * 4);
    check(nle_dev_upload(c, o.bgr.p, image.ptr<unsigned short>(), n * 6), c);
    check(nle_bgr16_to_lab(c, static_cast<const unsigned short*>(o.bgr.p), (long long)n, o.L.f(), o.a.f(), o.b.f(), o.guide.f()), c);
    return o;
}

// epilogue: d_L with in's a and b -> a 16UC3 image of the input's size; nothing is rounded before the 16-bit codes
inline Image lab16_to_image(nle_ctx* c, const Lab16Planes& in, const float* d_L, int rows, int cols) {
    Image out(rows, cols, NLE_16U, 3);
    const size_t n = out.total();
    check(nle_lab_to_bgr16(c, d_L, in.a.f(), in.b.f(), (long long)n, static_cast<unsigned short*>(in.bgr.p)), c);
    check(nle_dev_download(c, out.ptr<unsigned short>(), in.bgr.p, n * 6), c);
    return out;
}

// ---- HDR tone mapping (32FC3 linear-light images): the same two steps on log-luminance ----
// prologue: the image on the device and, on the scale (l_hi, range), x (the unrounded log-luminance plane) or the guide (x
// rounded to the 256 levels a train takes), whichever is wanted; with find_range the scale is first taken from the image
struct HdrPlanes {
    Dev bgr, x, guide;
    double l_hi = 0, range = 0;
};
inline HdrPlanes hdr_planes(nle_ctx* c, const Image& image, bool find_range, double l_hi, double range, bool want_x,
                            bool want_guide) {
    const size_t n = image.total();
    HdrPlanes o;
    o.bgr = Dev(c, n * 12);
    if (want_x) o.x = Dev(c, n * 4);
    if (want_guide) o.guide = Dev(c, n * 4);
    check(nle_dev_upload(c, o.bgr.p, image.ptr<float>(), n * 12), c);
    if (find_range) check(nle_hdr_range(c, o.bgr.f(), (long long)n, &l_hi, &range), c);
    o.l_hi = l_hi;
    o.range = range;
    check(nle_hdr_to_loglum(c, o.bgr.f(), (long long)n, l_hi, range, o.x.f(), o.guide.f()), c);
    return o;
}

// epilogue: the filtered plane d_y with in's colours -> a 16UC3 sRGB image of the input's size
inline Image hdr_to_image(nle_ctx* c, const HdrPlanes& in, const float* d_y, double base_weight, double saturation, int rows,
                          int cols) {
    Image out(rows, cols, NLE_16U, 3);
    const size_t n = out.total();
    Dev d_out(c, n * 6);
    check(nle_loglum_to_bgr16(c, d_y, in.bgr.f(), (long long)n, in.l_hi, in.range, base_weight, saturation,
                              static_cast<unsigned short*>(d_out.p)), c);
    check(nle_dev_download(c, out.ptr<unsigned short>(), d_out.p, n * 6), c);
    return out;
}

}  // namespace nle::surface
