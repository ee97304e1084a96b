// NLEFilter of the C++ drop-in surface (include/nle/filter.hpp) over the C ABI (include/nle.h): the reference's class,
// src/filter.cpp:349-538, method by method.  Every N-sized product runs in libnle_hip.so on the GPU; what the methods
// repeat -- ctx options, colour prologue and epilogue -- is owned by surface_internal.hpp, the NLE_DEVICES group by
// device_group.hpp.  A call runs one body either on the whole image or, under a group, on every rank's rows.
#include "nle/filter.hpp"

#include <algorithm>
#include <cmath>
#include <iostream>
#include <numeric>
#include <string>

#include "device_group.hpp"
#include "surface_internal.hpp"

namespace nle {

using namespace surface;

namespace {

const char kTrainedSize[] = "Cannot apply filter on image with different size from the image filter was trained on.";
const char kChannelSize[] = "Number of values in channel must match that of training image.";
const char kSampleCount[] = "Number of samples per row and col must be <= that of image.";

struct TrainArgs {
    int nRowSamples, nColSamples;
    DType hx, hy;
    int nSinkhornIter, nEigenVectors;
};

// the train step: the filter's options on ctx c for the length of nle_train, whatever comes of it
nle_filter* train_step(nle_ctx* c, const NLEFilter& o, const float* d_lum, int rows, int cols, const TrainArgs& a,
                       const float* d_a, const float* d_b) {
    TrainOptions options(c, o, d_a, d_b);
    nle_filter* f = nullptr;
    check(nle_train(c, d_lum, rows, cols, a.nRowSamples, a.nColSamples, a.hx, a.hy, a.nSinkhornIter, a.nEigenVectors, &f), c);
    return f;
}

// a device buffer handed over to shared ownership (the copies of an NLEFilter share what its train left)
std::shared_ptr<void> keep_plane(Dev& d) {
    nle_ctx* c = d.c;
    void* p = d.p;
    d.p = nullptr;
    return std::shared_ptr<void>(p, [c](void* q) {
        if (q) nle_dev_free(c, q);
    });
}

// rows [r0, r1) of a BGR image -- all of it, or a rank's slab (slab input: the train still takes the image's size) --
// on ctx c: getLuminanceChannel (:460-469) on the device, BGR -> Lab (8 bit) -> L as float (and the a and b planes of
// the same Lab image, alive for the train, when the filter has a chroma bandwidth), then the train step.  Under a group
// a patch radius, a sampler other than the grid, the exact mode and chroma are refused by the train (world > 1).
// keepL (may be null) receives the L plane after the train: what NLEFilter::segment starts from.
nle_filter* train_rows(nle_ctx* c, const NLEFilter& o, const Image& image, int r0, int r1, const TrainArgs& a,
                       std::shared_ptr<void>* keepL) {
    const bool chroma = o.chromaBandwidth != 0;
    LabPlanes in = lab_planes(c, image.ptr<unsigned char>(r0), (size_t)(r1 - r0) * image.cols, chroma, chroma);
    nle_filter* f = train_step(c, o, in.L.f(), image.rows, image.cols, a, in.a.f(), in.b.f());
    if (keepL) *keepL = keep_plane(in.L);
    return f;
}

// One luminance edit per image kind.  The kind fixes the prologue and the epilogue; `op(d_x, d_y)` is the operator on the
// plane: it fills the floats at d_y from those at d_x (nle_apply / nle_apply_rounded8, nle_apply_detail, nle_apply_regions)
// and does its own check().
// 8 bit, rows [r0, r1) of `image` on ctx c into the same rows of `out` (:422-440 on the device): BGR -> Lab, L -> float, op
// (which clamps and rounds to 8 bit), merge with a, b, Lab -> BGR
template <typename Op>
void edit_rows(nle_ctx* c, const Image& image, int r0, int r1, Image& out, Op&& op) {
    const size_t n = (size_t)(r1 - r0) * image.cols;
    const LabPlanes in = lab_planes(c, image.ptr<unsigned char>(r0), n, true, false);
    Dev d_y(c, n * 4);
    op(in.L.f(), d_y.f());
    lab_to_rows(c, in, d_y.f(), nullptr, nullptr, out, r0, r1);
}

// ... the whole image
template <typename Op>
Image edit_8bit(nle_ctx* c, const Image& image, Op&& op) {
    Image out(image.rows, image.cols, NLE_8U, 3);
    edit_rows(c, image, 0, image.rows, out, op);
    return out;
}

// deep colour: float Lab in, op on the unrounded L, 16-bit codes out; nothing is rounded to 8 bit
template <typename Op>
Image edit_deep(nle_ctx* c, const Image& image, Op&& op) {
    const Lab16Planes in = lab16_planes(c, image, true, false);
    Dev d_y(c, image.total() * 4);
    op(in.L.f(), d_y.f());
    return lab16_to_image(c, in, d_y.f(), image.rows, image.cols);
}

// the same two edits with an operator that also sees the chroma planes: op(d_x, d_y, d_a, d_b) may rewrite a and b in place.
// 8 bit without `chroma`: a and b are not made (op gets null pointers) and the edit is edit_8bit's, byte for byte
template <typename Op>
Image edit_8bit_lab(nle_ctx* c, const Image& image, bool chroma, Op&& op) {
    Image out(image.rows, image.cols, NLE_8U, 3);
    const size_t n = image.total();
    const LabPlanes in = lab_planes(c, image.ptr<unsigned char>(), n, true, chroma);
    Dev d_y(c, n * 4);
    op(in.L.f(), d_y.f(), in.a.f(), in.b.f());
    lab_to_rows(c, in, d_y.f(), in.a.f(), in.b.f(), out, 0, image.rows);
    return out;
}

template <typename Op>
Image edit_deep_lab(nle_ctx* c, const Image& image, Op&& op) {
    const Lab16Planes in = lab16_planes(c, image, true, false);
    Dev d_y(c, image.total() * 4);
    op(in.L.f(), d_y.f(), in.a.f(), in.b.f());
    return lab16_to_image(c, in, d_y.f(), image.rows, image.cols);
}

// HDR: the unrounded log-luminance on the scale of the train (hi, range), op, then base compression and saturation
template <typename Op>
Image edit_hdr(nle_ctx* c, const Image& image, double hi, double range, DType base, DType saturation, Op&& op) {
    const HdrPlanes in = hdr_planes(c, image, false, hi, range, true, false);
    Dev d_y(c, image.total() * 4);
    op(in.x.f(), d_y.f());
    return hdr_to_image(c, in, d_y.f(), base, saturation, image.rows, image.cols);
}

// rows [r0, r1) through filter f of ctx c: the plain enhance of a rank's rows, or of all of them (:431-436)
void enhance_rows(nle_ctx* c, nle_filter* f, const Image& image, const Vec& fS, int r0, int r1, Image& out) {
    edit_rows(c, image, r0, r1, out, [&](const float* d_x, float* d_y) {
        check(nle_apply_rounded8(f, d_x, image.rows, image.cols, fS.data(), d_y), c);
    });
}

const char kDeepOneDevice[] = "Deep colour (16-bit images) runs on one device: unset NLE_DEVICES.";

bool is_deep(const Image& image) { return image.channels() == 3 && image.depth() == NLE_16U; }

// HDR (32F) images have their own pair of methods; every other one refuses them by name
const char kHdrOneDevice[] = "Tone mapping runs on one device: unset NLE_DEVICES.";
const char kHdrNoChroma[] = "Tone mapping does not take chroma affinities (chromaBandwidth must be 0): a linear-light image has no 8-bit a and b planes.";
void refuse_hdr(const Image& image, const char* method) {
    if (image.depth() == NLE_32F)
        throw std::runtime_error(std::string(method) + " does not take a 32F (HDR) image: use trainForToneMapping and toneMap.");
}

// The planes a deep-colour train (or residual map) takes: the guide for L and, with a chroma bandwidth, a and b rounded
// half to even and clamped to [0, 255] like the guide -- the chroma affinity sums integer differences (nle_ctx_set_chroma).
// The rounding of these two opt-in planes is done on the host.
struct DeepChroma {
    Dev a, b;
};
DeepChroma deep_chroma_planes(nle_ctx* c, const Lab16Planes& in, size_t n, bool chroma) {
    DeepChroma o;
    if (!chroma) return o;
    std::vector<float> h(2 * n);
    check(nle_dev_download(c, h.data(), in.a.p, n * 4), c);
    check(nle_dev_download(c, h.data() + n, in.b.p, n * 4), c);
    for (float& v : h) v = std::fmin(255.f, std::fmax(0.f, std::nearbyint(v)));
    o.a = Dev(c, n * 4);
    o.b = Dev(c, n * 4);
    check(nle_dev_upload(c, o.a.p, h.data(), n * 4), c);
    check(nle_dev_upload(c, o.b.p, h.data() + n, n * 4), c);
    return o;
}

// fn(ctx, rank, r0, r1) on every rank's rows of an H-row image, one thread per rank of the group; without a group
// here, on all rows, on ctx c
template <typename Fn>
void on_rows(DeviceGroup* g, nle_ctx* c, int H, Fn&& fn) {
    if (!g) return fn(c, 0, 0, H);
    g->run([&](int r) {
        int r0 = 0, r1 = 0;
        check(nle_slab_rows(H, r, g->size(), &r0, &r1), g->ctx[r]);
        fn(g->ctx[r], r, r0, r1);
    });
}

}  // namespace

NLEFilter::NLEFilter() = default;
NLEFilter::~NLEFilter() = default;

long long NLEFilter::n_local() const {
    long long n = 0;
    if (f_) nle_filter_info(f_, &n, nullptr, nullptr, nullptr, nullptr, nullptr);
    return n;
}

int NLEFilter::K() const {
    int k = 0;
    if (f_) nle_filter_info(f_, nullptr, &k, nullptr, nullptr, nullptr, nullptr);
    return k;
}

void NLEFilter::requireSize(size_t pixels, const char* message) const {
    if (!f_ || (long long)pixels != n_local()) throw std::runtime_error(message);
}

void NLEFilter::beginTrain(nle_ctx* c) {
    ctx_ = c;
    fh_.reset();
    f_ = nullptr;
    group_.clear();
    hdrHi_ = hdrRange_ = 0;  // trainForToneMapping sets them after its train
    denoiseTrained_ = false;  // trainForDenoise likewise
    denoiseReport_ = DenoiseReport();
    trainPlane_.reset();  // trainForEnhancement sets it after its train; a segmentation belongs to the filter it was made on
    segmentSpreads_.reset();
    segmentCount_ = 0;
    segmentReport_ = SegmentReport();
    if (verbose) {
        // the four stages run as one fused GPU pipeline; the banners keep the reference's stdout (:483-498)
        std::cout << "Computing kernel" << std::endl;
        std::cout << "Nystrom approximation" << std::endl;
        std::cout << "Sinkhorn" << std::endl;
        std::cout << "Orthogonalize" << std::endl;
    }
}

void NLEFilter::adopt(const std::vector<nle_ctx*>& ctxs, const std::vector<nle_filter*>& fs, int rows, int cols,
                      int nEigenVectors) {
    std::vector<std::shared_ptr<nle_filter>> hs;
    for (nle_filter* f : fs) hs.emplace_back(f, [](nle_filter* p) { nle_filter_destroy(p); });
    ctx_ = ctxs[0];
    fh_ = hs[0];
    f_ = fh_.get();
    rows_ = rows;
    cols_ = cols;
    if (hs.size() > 1) group_ = std::move(hs);
    if (!verbose) return;
    const Vec ev = eigvals();
    const int nshow = std::min(std::min(nEigenVectors, 5), ev.size());  // :504-506 (imshow dropped)
    double mn[5], mx[5];
    for (size_t r = 0; r < fs.size() && nshow > 0; ++r) {  // min / max on the device, over the ranks' slabs
        double a[5], b[5];
        check(nle_filter_eigvec_range(fs[r], nshow, a, b), ctxs[r]);
        for (int i = 0; i < nshow; ++i) {
            mn[i] = r ? std::min(mn[i], a[i]) : a[i];
            mx[i] = r ? std::max(mx[i], b[i]) : b[i];
        }
    }
    for (int i = 0; i < nshow; i++)
        std::cout << "Eigvec " << i << " eigval: " << ev(i) << " minCoeff: " << mn[i] << " maxCoeff: " << mx[i] << std::endl;
}

void NLEFilter::trainFilter(const Image& channel, int nRowSamples, int nColSamples, DType hx, DType hy,
                            int nSinkhornIter, int nEigenVectors) {  // :480-512
    if (nRowSamples > channel.rows || nColSamples > channel.cols) throw std::runtime_error(kSampleCount);
    const Dev d_lum = upload_plane(shared_ctx(), channel);
    trainOnDevice(d_lum.f(), channel.rows, channel.cols, nRowSamples, nColSamples, hx, hy, nSinkhornIter, nEigenVectors);
}

void NLEFilter::trainOnDevice(const float* d_lum, int rows, int cols, int nRowSamples, int nColSamples, DType hx,
                              DType hy, int nSinkhornIter, int nEigenVectors, const float* d_a, const float* d_b) {
    nle_ctx* c = shared_ctx();
    const TrainArgs a{nRowSamples, nColSamples, hx, hy, nSinkhornIter, nEigenVectors};
    beginTrain(c);
    adopt({c}, {train_step(c, *this, d_lum, rows, cols, a, d_a, d_b)}, rows, cols, nEigenVectors);
}

void NLEFilter::trainForEnhancement(const Image& image, int nRowSamples, int nColSamples, DType hx, DType hy,
                                    int nSinkhornIter, int nEigenVectors) {  // :514-519
    refuse_hdr(image, "trainForEnhancement");
    if (image.channels() != 3 || (image.depth() != NLE_8U && image.depth() != NLE_16U))
        throw std::runtime_error("Can only enhance RGB image.");
    if (nRowSamples > image.rows || nColSamples > image.cols) throw std::runtime_error(kSampleCount);
    if (is_deep(image)) {
        // deep colour: 16-bit sRGB -> float Lab on the device, then the train on the guide (L rounded to 256 levels: the
        // default table path, and the affinities need no more); enhance applies the filter to the unrounded L
        // as for 8-bit images a group forms only when NLE_DEVICES lists two devices or more
        if (devices_env() != nullptr && device_group(-1) != nullptr) throw std::runtime_error(kDeepOneDevice);
        nle_ctx* c = shared_ctx();
        Lab16Planes in = lab16_planes(c, image, chromaBandwidth != 0, true);
        const DeepChroma ab = deep_chroma_planes(c, in, image.total(), chromaBandwidth != 0);
        trainOnDevice(in.guide.f(), image.rows, image.cols, nRowSamples, nColSamples, hx, hy, nSinkhornIter, nEigenVectors,
                      ab.a.f(), ab.b.f());
        if (keepTrainPlane) trainPlane_ = keep_plane(in.guide);
        return;
    }
    const TrainArgs a{nRowSamples, nColSamples, hx, hy, nSinkhornIter, nEigenVectors};
    const int H = image.rows, W = image.cols;
    DeviceGroup* g = nullptr;
    if (devices_env() != nullptr) {
        int rs, ro, nr, cs, co, nc;
        if (nle_sample_grid(H, W, nRowSamples, nColSamples, &rs, &ro, &nr, &cs, &co, &nc) == NLE_OK) g = device_group(nr * nc);
    }
    // NLE_DEVICES: the image by row slabs over the group (slab input), rank r's filter is group_[r]
    if (g && g->size() > H) throw std::runtime_error("more devices than image rows");
    const std::vector<nle_ctx*> ctxs = g ? g->ctx : std::vector<nle_ctx*>{shared_ctx()};
    beginTrain(ctxs[0]);
    std::vector<nle_filter*> fs(ctxs.size(), nullptr);
    std::shared_ptr<void> plane;  // one device, on request: the L plane stays for segment()
    on_rows(g, ctxs[0], H, [&](nle_ctx* c, int r, int r0, int r1) {
        fs[r] = train_rows(c, *this, image, r0, r1, a, !g && keepTrainPlane ? &plane : nullptr);
    });
    adopt(ctxs, fs, H, W, nEigenVectors);
    trainPlane_ = plane;
}

void NLEFilter::trainForToneMapping(const Image& image, int nRowSamples, int nColSamples, DType hx, DType hy, int nSinkhornIter,
                                    int nEigenVectors) {
    if (image.channels() != 3 || image.depth() != NLE_32F) throw std::runtime_error("Can only tone-map a 32F RGB image.");
    if (nRowSamples > image.rows || nColSamples > image.cols) throw std::runtime_error(kSampleCount);
    if (chromaBandwidth != 0) throw std::runtime_error(kHdrNoChroma);
    // as for 8-bit images a group forms only when NLE_DEVICES lists two devices or more
    if (devices_env() != nullptr && device_group(-1) != nullptr) throw std::runtime_error(kHdrOneDevice);
    // the image's range, log-luminance on the scale of an L plane, then the train on its guide (256 levels: the default
    // table path); toneMap applies the filter to the unrounded plane on the same scale
    nle_ctx* c = shared_ctx();
    const HdrPlanes in = hdr_planes(c, image, true, 0, 0, false, true);
    trainOnDevice(in.guide.f(), image.rows, image.cols, nRowSamples, nColSamples, hx, hy, nSinkhornIter, nEigenVectors);
    hdrHi_ = in.l_hi;
    hdrRange_ = in.range;
}

Image NLEFilter::toneMap(const Image& image, const std::vector<DType>& weights, DType saturation) const {
    return toneMap(image, weights, saturation, DetailOptions());
}

void NLEFilter::trainForDenoise(const Image& image, int nRowSamples, int nColSamples, DType hx, DType hy,
                                int nSinkhornIter, int nEigenVectors, int sigmaColor, int sigmaSpace) {  // :521-538
    trainForDenoise(image, nRowSamples, nColSamples, hx, hy, nSinkhornIter, nEigenVectors, sigmaColor, sigmaSpace, DenoiseOptions());
}

Image NLEFilter::denoise(const Image& image, DType k, int sigmaColor, int sigmaSpace) const {  // :349-410
    return denoise(image, k, sigmaColor, sigmaSpace, DenoiseOptions());
}

namespace {
const char kDenoiseOneDevice[] = "The denoise options (NLM pre-filter, glide) run on one device: unset NLE_DEVICES.";
bool default_options(const DenoiseOptions& o) { return o.prefilter == NLE_PREFILTER_BILATERAL && !o.glide; }
}  // namespace

void NLEFilter::trainForDenoise(const Image& image, int nRowSamples, int nColSamples, DType hx, DType hy, int nSinkhornIter,
                                int nEigenVectors, int sigmaColor, int sigmaSpace, const DenoiseOptions& options) {
    refuse_hdr(image, "trainForDenoise");
    if (is_deep(image)) throw std::runtime_error("Denoise takes an 8-bit image: deep colour (16 bit) is built for enhance only.");
    if (image.channels() != 3 || image.depth() != NLE_8U) throw std::runtime_error("Can only enchance RGB image.");
    if (nRowSamples > image.rows || nColSamples > image.cols) throw std::runtime_error(kSampleCount);
    if (chromaBandwidth != 0)
        throw std::runtime_error("trainForDenoise does not take chroma affinities (chromaBandwidth must be 0): the a and b "
                                 "planes are what it estimates");
    if (!default_options(options)) {
        check_denoise_options(options, sigmaColor, sigmaSpace);
        if (devices_env() != nullptr && device_group(-1) != nullptr) throw std::runtime_error(kDenoiseOneDevice);
    }
    // BGR -> Lab, L, the pre-filter (8 bit: the bilateral filter, or non-local means), convertTo(double), trainFilter -- all on
    // the device
    nle_ctx* c = shared_ctx();
    const LabPlanes in = lab_planes(c, image.ptr<unsigned char>(), image.total(), false, false);
    Dev d_Y(c, image.total() * 4);
    const double sigma = options.prefilter == NLE_PREFILTER_NLM ? plane_sigma(c, options, in.L.f(), image.rows, image.cols) : 0;
    prefilter_plane(c, options, in.L.f(), image.rows, image.cols, sigmaColor, sigmaSpace, sigma, d_Y.f());
    trainOnDevice(d_Y.f(), image.rows, image.cols, nRowSamples, nColSamples, hx, hy, nSinkhornIter, nEigenVectors);
    denoiseTrained_ = true;
}

Image NLEFilter::denoise(const Image& image, DType k, int sigmaColor, int sigmaSpace, const DenoiseOptions& options) const {
    refuse_hdr(image, "denoise");
    if (image.channels() != 3) throw std::runtime_error("Can only enchance RGB image.");  // (sic) :351-353
    if (is_deep(image)) throw std::runtime_error("Denoise takes an 8-bit image: deep colour (16 bit) is built for enhance only.");
    requireSize(image.total(), kTrainedSize);
    if (image.depth() != NLE_8U) throw std::runtime_error("Can only enchance RGB image.");
    if (!default_options(options)) {
        check_denoise_options(options, sigmaColor, sigmaSpace);
        if (!group_.empty()) throw std::runtime_error(kDenoiseOneDevice);
        if (options.glide && !denoiseTrained_) throw std::runtime_error("denoise with glide needs a filter trained by trainForDenoise.");
        if (options.glide && (!std::isfinite(k) || k < 0))
            throw std::runtime_error("denoise with glide searches k on [0, shrink factor]: the shrink factor must be finite and >= 0.");
    }
    const size_t np = image.total();
    const int H = image.rows, W = image.cols;
    const LabPlanes in = lab_planes(ctx_, image.ptr<unsigned char>(), np, true, false);
    Image out(H, W, NLE_8U, 3);
    const Vec ev = eigvals();
    const int K = ev.size();
    if (options.glide) {
        // L, a and b of the noisy image; their noise levels; all three pre-filtered; the coefficients of the pre-filtered
        // planes choose k per plane; the filter then runs on the noisy planes, L included
        Dev d_noisy(ctx_, 3 * np * 4), d_pre(ctx_, 3 * np * 4), d_out(ctx_, 3 * np * 4);
        DenoiseReport rep;
        for (int ch = 0; ch < 3; ++ch) {
            check(nle_lab8_channel(ctx_, in.lab.u8(), (long long)np, ch, d_noisy.f() + (size_t)ch * np), ctx_);
            rep.sigma[ch] = plane_sigma(ctx_, options, d_noisy.f() + (size_t)ch * np, H, W);
            prefilter_plane(ctx_, options, d_noisy.f() + (size_t)ch * np, H, W, sigmaColor, sigmaSpace, rep.sigma[ch],
                            d_pre.f() + (size_t)ch * np);
        }
        std::vector<double> b((size_t)3 * K), resp((size_t)3 * K), mse(257);
        check(nle_filter_coefficients(f_, d_pre.f(), 3, (long long)np, H, W, b.data()), ctx_);
        for (int ch = 0; ch < 3; ++ch) {
            if (nle_mse_shrink(ev.data(), b.data() + (size_t)ch * K, K, rep.sigma[ch], k, 256, &rep.k[ch], mse.data()) != NLE_OK)
                throw std::runtime_error("nle_mse_shrink refused its arguments");
            rep.mse[ch] = *std::min_element(mse.begin(), mse.end());
            for (int i = 0; i < K; ++i) resp[(size_t)ch * K + i] = std::pow(std::min(std::max(ev(i), 0.0), 1.0), rep.k[ch]);
        }
        if (verbose)
            for (int i = 0; i < K; ++i) std::cout << "eig " << i << " val: " << std::min(ev(i), 1.0) << std::endl;
        check(nle_apply_planes(f_, d_noisy.f(), 3, (long long)np, H, W, nullptr, resp.data(), NLE_REGION_OUT_ROUNDED8, d_out.f(),
                               (long long)np), ctx_);
        lab_to_rows(ctx_, in, d_out.f(), d_out.f() + np, d_out.f() + 2 * np, out, 0, H);
        rep.valid = true;
        denoiseReport_ = rep;
        return out;
    }
    Dev d_Y(ctx_, np * 4), d_c(ctx_, np * 8), d_ab(ctx_, np * 8);
    // the L channel becomes its pre-filtered version (:370-373; `apply` on it is commented out, :389)
    const double sigma = options.prefilter == NLE_PREFILTER_NLM ? plane_sigma(ctx_, options, in.L.f(), H, W) : 0;
    prefilter_plane(ctx_, options, in.L.f(), H, W, sigmaColor, sigmaSpace, sigma, d_Y.f());
    Vec t = ev;
    for (int i = 0; i < t.size(); ++i) {  // :380-387
        const DType e = std::min(t(i), 1.0);
        if (verbose) std::cout << "eig " << i << " val: " << e << std::endl;
        t(i) = std::pow(e, k);
    }
    // a and b through the filter in one call (:390-391, + :394-399): two planes, the same response, rounded as
    // nle_apply_rounded8 rounds
    for (int ch = 1; ch <= 2; ++ch)
        check(nle_lab8_channel(ctx_, in.lab.u8(), (long long)np, ch, d_c.f() + (size_t)(ch - 1) * np), ctx_);
    std::vector<double> t2((size_t)2 * t.size());
    for (int i = 0; i < t.size(); ++i) t2[i] = t2[(size_t)t.size() + i] = t(i);
    check(nle_apply_planes(f_, d_c.f(), 2, (long long)np, H, W, nullptr, t2.data(), NLE_REGION_OUT_ROUNDED8, d_ab.f(),
                           (long long)np), ctx_);
    // max(0) / min(255) / convertTo(CV_8U) of the three planes, merge, Lab -> BGR (:393-409)
    lab_to_rows(ctx_, in, d_Y.f(), d_ab.f(), d_ab.f() + np, out, 0, H);
    return out;
}

Image NLEFilter::apply(const Image& channel, const Vec& transformedEigVals) const {  // :445-458
    requireSize(channel.total(), kChannelSize);
    if (transformedEigVals.size() != K()) throw std::runtime_error("apply: one transformed eigenvalue per eigenvector expected");
    std::vector<float> x = plane_f32(channel), y(channel.total());
    check(nle_apply_host(f_, x.data(), channel.rows, channel.cols, transformedEigVals.data(), y.data()), ctx_);
    return image_f64(y.data(), channel.rows, channel.cols);
}

std::vector<Image> NLEFilter::applyPlanes(const std::vector<Image>& channels,
                                          const std::vector<std::vector<Vec>>& responses) const {
    if (!f_ || channels.empty() || channels.size() != responses.size())
        throw std::runtime_error("applyPlanes: one set of responses per channel expected");
    const int nK = K(), rows = channels[0].rows, cols = channels[0].cols;
    const size_t P = channels.size(), N = channels[0].total();
    std::vector<int> nresp(P);
    std::vector<double> resp;
    std::vector<float> x(P * N);
    for (size_t m = 0; m < P; ++m) {
        requireSize(channels[m].total(), kChannelSize);
        if (channels[m].rows != rows || channels[m].cols != cols) throw std::runtime_error(kChannelSize);
        nresp[m] = (int)responses[m].size();
        for (const Vec& r : responses[m]) {
            if (r.size() != nK) throw std::runtime_error("applyPlanes: one transformed eigenvalue per eigenvector expected");
            resp.insert(resp.end(), r.data(), r.data() + nK);
        }
        const std::vector<float> xm = plane_f32(channels[m]);
        std::copy(xm.begin(), xm.end(), x.begin() + m * N);
    }
    const size_t R = nK > 0 ? resp.size() / (size_t)nK : 0;
    Dev d_x(ctx_, P * N * 4), d_y(ctx_, std::max<size_t>(R, 1) * N * 4);
    check(nle_dev_upload(ctx_, d_x.p, x.data(), P * N * 4), ctx_);
    check(nle_apply_planes(f_, d_x.f(), (int)P, (long long)N, rows, cols, nresp.data(), resp.data(), NLE_REGION_OUT_F32,
                           d_y.f(), (long long)N), ctx_);
    std::vector<float> y(R * N);
    check(nle_dev_download(ctx_, y.data(), d_y.p, R * N * 4), ctx_);
    std::vector<Image> out;
    for (size_t j = 0; j < R; ++j) out.push_back(image_f64(y.data() + j * N, rows, cols));
    return out;
}

std::vector<Image> NLEFilter::applyLayers(const Image& channel, int nLayers) const {
    requireSize(channel.total(), kChannelSize);
    std::vector<float> x = plane_f32(channel), y((size_t)nLayers * channel.total());
    check(nle_apply_layers_host(f_, x.data(), channel.rows, channel.cols, nLayers, y.data()), ctx_);
    std::vector<Image> out;
    for (int l = 0; l < nLayers; ++l) out.push_back(image_f64(y.data() + (size_t)l * channel.total(), channel.rows, channel.cols));
    return out;
}

Image NLEFilter::enhance(const Image& image, const std::vector<DType>& weights) const {  // :412-443
    refuse_hdr(image, "enhance");
    if (image.channels() != 3) throw std::runtime_error("Can only enhance RGB image.");
    const int H = image.rows, W = image.cols;
    if (is_deep(image)) {
        if (!group_.empty()) throw std::runtime_error(kDeepOneDevice);
        requireSize(image.total(), kTrainedSize);
        const Vec fS = transformEigenValues(eigvals(), weights);
        return edit_deep(ctx_, image, [&](const float* d_x, float* d_y) { check(nle_apply(f_, d_x, H, W, fS.data(), d_y), ctx_); });
    }
    DeviceGroup* g = nullptr;
    if (!group_.empty()) {  // trained over NLE_DEVICES: every rank its rows
        if (image.depth() != NLE_8U) throw std::runtime_error("Can only enhance RGB image.");
        g = device_group(-1);
        if (!g || (int)group_.size() != g->size() || H != rows_ || W != cols_) throw std::runtime_error(kTrainedSize);
    } else {
        requireSize(image.total(), kTrainedSize);
        if (image.depth() != NLE_8U) throw std::runtime_error("Can only enhance RGB image.");
    }
    const Vec fS = transformEigenValues(eigvals(), weights);
    Image out(H, W, NLE_8U, 3);
    on_rows(g, ctx_, H, [&](nle_ctx* c, int r, int r0, int r1) {
        enhance_rows(c, g ? group_[r].get() : f_, image, fS, r0, r1, out);
    });
    return out;
}

namespace {

const char kDetailOneDevice[] = "DetailOptions (residualWeight, gain, sigma) run on one device: this filter was trained on a device group (NLE_DEVICES).";

// the layer count of a call with active DetailOptions
int detail_layers(const std::vector<DType>& weights) {
    if (weights.empty() || (int)weights.size() > NLE_REGION_LAYERS_MAX)
        throw std::runtime_error("DetailOptions take 1 to " + std::to_string(NLE_REGION_LAYERS_MAX) + " weights.");
    return (int)weights.size();
}

// nle_apply_detail as the operator of a luminance edit (the weight count is refused here, before the edit begins)
auto detail_op(nle_ctx* c, nle_filter* f, const Image& image, const std::vector<DType>& weights, const DetailOptions& detail,
               int out_kind) {
    const int H = image.rows, W = image.cols, L = detail_layers(weights);
    return [=, &weights](const float* d_x, float* d_y) {
        check(nle_apply_detail(f, d_x, H, W, L, weights.data(), detail.residualWeight, detail.gain, detail.sigma, out_kind, d_y), c);
    };
}

}  // namespace

Image NLEFilter::enhance(const Image& image, const std::vector<DType>& weights, const DetailOptions& detail) const {
    if (!detail.active()) return enhance(image, weights);
    refuse_hdr(image, "enhance");
    if (image.channels() != 3 || (image.depth() != NLE_8U && image.depth() != NLE_16U))
        throw std::runtime_error("Can only enhance RGB image.");
    if (!group_.empty()) throw std::runtime_error(kDetailOneDevice);
    requireSize(image.total(), kTrainedSize);
    if (is_deep(image)) return edit_deep(ctx_, image, detail_op(ctx_, f_, image, weights, detail, NLE_REGION_OUT_F32));
    return edit_8bit(ctx_, image, detail_op(ctx_, f_, image, weights, detail, NLE_REGION_OUT_ROUNDED8));
}

// nle_apply_tone as the operator of the same edits; the curve's range is kept for lastToneCurve()
Image NLEFilter::enhance(const Image& image, const std::vector<DType>& weights, const DetailOptions& detail,
                         const ToneOptions& tone) const {
    if (!tone.active()) return enhance(image, weights, detail);
    refuse_hdr(image, "enhance");
    if (image.channels() != 3 || (image.depth() != NLE_8U && image.depth() != NLE_16U))
        throw std::runtime_error("Can only enhance RGB image.");
    if (!group_.empty())
        throw std::runtime_error("ToneOptions (shadows, highlights, clipPercent, equalise) run on one device: this filter was trained on a device group (NLE_DEVICES).");
    requireSize(image.total(), kTrainedSize);
    const int H = image.rows, W = image.cols, L = detail_layers(weights);
    const bool deep = is_deep(image);
    std::vector<double> curve(NLE_TONE_KNOTS + 2);
    const auto op = [&](const float* d_x, float* d_y) {
        check(nle_apply_tone(f_, d_x, H, W, L, weights.data(), detail.residualWeight, detail.gain, detail.sigma, tone.shadows,
                             tone.highlights, tone.clipPercent, tone.equalise, deep ? NLE_REGION_OUT_F32 : NLE_REGION_OUT_ROUNDED8,
                             d_y, curve.data()),
              ctx_);
    };
    Image out = deep ? edit_deep(ctx_, image, op) : edit_8bit(ctx_, image, op);
    toneLevels_.lo = curve[0], toneLevels_.hi = curve[1], toneLevels_.valid = true;
    return out;
}

// inactive options: the plain toneMap, nle_apply under the transformed eigenvalues (the one-device and the weight-count
// refusals keep each form's own text)
Image NLEFilter::toneMap(const Image& image, const std::vector<DType>& weights, DType saturation,
                         const DetailOptions& detail) const {
    const bool plain = !detail.active();
    if (image.channels() != 3 || image.depth() != NLE_32F) throw std::runtime_error("Can only tone-map a 32F RGB image.");
    if (chromaBandwidth != 0) throw std::runtime_error(kHdrNoChroma);
    if (!group_.empty()) throw std::runtime_error(plain ? kHdrOneDevice : kDetailOneDevice);
    requireSize(image.total(), kTrainedSize);
    if (!(hdrRange_ > 0)) throw std::runtime_error("toneMap needs a filter trained by trainForToneMapping.");
    if (!plain) {
        const auto op = detail_op(ctx_, f_, image, weights, detail, NLE_REGION_OUT_F32);
        return edit_hdr(ctx_, image, hdrHi_, hdrRange_, weights.back(), saturation, op);  // c = f(1): the base weight
    }
    if (weights.empty()) throw std::runtime_error("toneMap needs at least one layer weight.");
    const Vec fS = transformEigenValues(eigvals(), weights);
    return edit_hdr(ctx_, image, hdrHi_, hdrRange_, weights.back(), saturation, [&](const float* d_x, float* d_y) {
        check(nle_apply(f_, d_x, image.rows, image.cols, fS.data(), d_y), ctx_);
    });
}

Image NLEFilter::enhanceRegions(const Image& image, const std::vector<Image>& strokes,
                                 const std::vector<std::vector<DType>>& regionWeights, const std::vector<DType>& weights,
                                 DType spread, DType floor) const {
    refuse_hdr(image, "enhanceRegions");
    if (is_deep(image)) throw std::runtime_error("Region edits take an 8-bit image: deep colour (16 bit) is built for enhance only.");
    if (image.channels() != 3 || image.depth() != NLE_8U) throw std::runtime_error("Can only enhance RGB image.");
    if (!group_.empty())
        throw std::runtime_error("Region edits run on one device: this filter was trained on a device group (NLE_DEVICES).");
    requireSize(image.total(), kTrainedSize);
    const int M = (int)strokes.size(), L = (int)weights.size();
    if (M < 1 || M > NLE_REGION_MAX)
        throw std::runtime_error("Region edits take 1 to " + std::to_string(NLE_REGION_MAX) + " strokes.");
    if (L < 1 || L > NLE_REGION_LAYERS_MAX)
        throw std::runtime_error("Region edits take 1 to " + std::to_string(NLE_REGION_LAYERS_MAX) + " weights.");
    if ((int)regionWeights.size() != M) throw std::runtime_error("Region edits need one weight vector per stroke.");
    const size_t np = image.total();
    // Wt: row 0 the background, row m region m; the stroke planes as 0 / 1 and their scales c_m = N / sum s_m
    std::vector<double> Wt(weights), scale((size_t)M);
    std::vector<float> planes((size_t)M * np);
    for (int m = 0; m < M; ++m) {
        if ((int)regionWeights[m].size() != L)
            throw std::runtime_error("Region " + std::to_string(m + 1) + " has " + std::to_string(regionWeights[m].size()) +
                                     " weights, the background has " + std::to_string(L) + ".");
        Wt.insert(Wt.end(), regionWeights[m].begin(), regionWeights[m].end());
        const Image& s = strokes[m];
        if (s.channels() != 1 || s.depth() != NLE_8U || s.rows != image.rows || s.cols != image.cols)
            throw std::runtime_error("Stroke " + std::to_string(m + 1) + " must be a one-channel 8-bit image of the image's size.");
        const unsigned char* b = s.ptr<unsigned char>();
        double sum = 0.0;
        for (size_t i = 0; i < np; ++i) {
            const float v = b[i] >= 128 ? 1.f : 0.f;
            planes[(size_t)m * np + i] = v;
            sum += v;
        }
        if (!(sum > 0)) throw std::runtime_error("Stroke " + std::to_string(m + 1) + " is empty (no byte >= 128).");
        scale[m] = (double)np / sum;
    }
    Dev d_s(ctx_, planes.size() * 4);
    check(nle_dev_upload(ctx_, d_s.p, planes.data(), planes.size() * 4), ctx_);
    return edit_8bit(ctx_, image, [&](const float* d_x, float* d_y) {
        check(nle_apply_regions(f_, d_x, image.rows, image.cols, L, d_s.f(), M, scale.data(), spread, floor, Wt.data(),
                                NLE_REGION_OUT_ROUNDED8, d_y), ctx_);
    });
}

Image NLEFilter::segment(const SegmentOptions& o) {
    if (!f_) throw std::runtime_error("segment needs a trained filter.");
    if (!group_.empty())
        throw std::runtime_error("Automatic regions run on one device: this filter was trained on a device group (NLE_DEVICES).");
    if (!trainPlane_)
        throw std::runtime_error("segment needs a filter trained by trainForEnhancement with keepTrainPlane set (it starts from that plane).");
    const int C = o.count;
    if (C < 1 || C > NLE_REGION_MAX)
        throw std::runtime_error("Automatic regions take 1 to " + std::to_string(NLE_REGION_MAX) + " segments.");
    if (!std::isfinite(o.floor) || !(o.floor > 0)) throw std::runtime_error("The segment floor must be finite and > 0.");
    const size_t n = (size_t)rows_ * cols_;
    const float* d_x = static_cast<const float*>(trainPlane_.get());
    Dev d_labels(ctx_, n), d_q(ctx_, (size_t)C * n * 4);
    check(nle_segment_init(ctx_, d_x, (long long)n, C, d_labels.u8(), nullptr), ctx_);
    SegmentReport r;
    r.counts.assign(C, 0);
    r.meanL.assign(C, 0.0);
    std::vector<double> objective((size_t)std::max(o.maxIterations, 1)), sums(C);
    int converged = 0;
    check(nle_filter_segment(f_, rows_, cols_, C, o.spread, o.maxIterations, d_labels.u8(), d_q.f(), (long long)n, r.counts.data(),
                             objective.data(), &r.iterations, &converged), ctx_);
    // the mean L of a segment: the per-segment sums of the one plane (q_stride 0)
    check(nle_segment_stats(ctx_, d_x, C, (long long)n, 0, d_labels.u8(), r.counts.data(), sums.data()), ctx_);
    for (int c = 0; c < C; ++c) r.meanL[c] = r.counts[c] ? sums[c] / (double)r.counts[c] : 0.0;
    r.converged = converged != 0;
    r.objective = objective[r.iterations - 1];
    r.valid = true;
    Image labels(rows_, cols_, NLE_8U, 1);
    check(nle_dev_download(ctx_, labels.ptr<unsigned char>(), d_labels.p, n), ctx_);
    segmentSpreads_ = keep_plane(d_q);
    segmentCount_ = C;
    segmentFloor_ = o.floor;
    segmentReport_ = r;
    return labels;
}

Image NLEFilter::enhanceSegments(const Image& image, const std::vector<DType>& weights,
                                  const std::vector<std::vector<DType>>& segmentWeights) const {
    refuse_hdr(image, "enhanceSegments");
    if (is_deep(image)) throw std::runtime_error("Segment edits take an 8-bit image: deep colour (16 bit) is built for enhance only.");
    if (image.channels() != 3 || image.depth() != NLE_8U) throw std::runtime_error("Can only enhance RGB image.");
    if (!group_.empty())
        throw std::runtime_error("Automatic regions run on one device: this filter was trained on a device group (NLE_DEVICES).");
    requireSize(image.total(), kTrainedSize);
    if (!segmentSpreads_) throw std::runtime_error("enhanceSegments needs a segment() of this filter first.");
    const int C = segmentCount_, L = (int)weights.size();
    if (L < 1 || L > NLE_REGION_LAYERS_MAX)
        throw std::runtime_error("Segment edits take 1 to " + std::to_string(NLE_REGION_LAYERS_MAX) + " weights.");
    if ((int)segmentWeights.size() > C)
        throw std::runtime_error("Segment edits take at most one weight vector per segment (" + std::to_string(C) + ").");
    std::vector<double> Wt(weights);  // row 0 the background, row 1 + c segment c
    for (int c = 0; c < C; ++c) {
        const std::vector<DType>& w = c < (int)segmentWeights.size() && !segmentWeights[c].empty() ? segmentWeights[c] : weights;
        if ((int)w.size() != L)
            throw std::runtime_error("Segment " + std::to_string(c) + " has " + std::to_string(w.size()) +
                                     " weights, the background has " + std::to_string(L) + ".");
        Wt.insert(Wt.end(), w.begin(), w.end());
    }
    const long long n = (long long)image.total();
    const float* d_q = static_cast<const float*>(segmentSpreads_.get());
    Dev d_layers(ctx_, (size_t)L * n * 4);
    return edit_8bit(ctx_, image, [&](const float* d_x, float* d_y) {
        check(nle_apply_layers(f_, d_x, image.rows, image.cols, L, d_layers.f()), ctx_);
        check(nle_region_combine(ctx_, d_layers.f(), L, d_q, C, n, n, n, Wt.data(), segmentFloor_, NLE_REGION_OUT_ROUNDED8, d_y), ctx_);
    });
}

namespace {

// the M + 1 rows of a local edit as nle_local_combine / nle_local_chroma take them; row 0 the background
struct LocalRowsHost {
    int L = 0;
    std::vector<double> weights, detail, curves, saturation, tone;  // tone: (shadows, highlights, clipPercent, equalise) per row
    std::vector<int> curveOn, histOn;                                // histOn: the row has auto levels or equalise
    bool anyCurve = false, chroma = false, anyHist = false;
    // what lastLocalLevels() returns once the curves are known: `cv` (M + 1) x (NLE_TONE_KNOTS + 2)
    std::vector<ToneLevels> levels(const double* cv) const {
        std::vector<ToneLevels> out(histOn.size());
        for (size_t m = 0; m < histOn.size(); ++m)
            if (histOn[m]) out[m].lo = cv[m * (NLE_TONE_KNOTS + 2)], out[m].hi = cv[m * (NLE_TONE_KNOTS + 2) + 1], out[m].valid = true;
        return out;
    }
};

LocalRowsHost local_rows(const LocalEdit& background, const std::vector<const LocalEdit*>& edits) {
    LocalRowsHost r;
    r.L = (int)background.weights.size();
    if (r.L < 1 || r.L > NLE_REGION_LAYERS_MAX)
        throw std::runtime_error("Local adjustments take 1 to " + std::to_string(NLE_REGION_LAYERS_MAX) + " weights.");
    const size_t rows = edits.size() + 1;
    r.curves.assign(rows * (NLE_TONE_KNOTS + 2), 0.0);
    for (size_t m = 0; m < rows; ++m) {
        const LocalEdit& e = m == 0 ? background : *edits[m - 1];
        const std::vector<DType>& w = e.weights.empty() ? background.weights : e.weights;
        if ((int)w.size() != r.L)
            throw std::runtime_error("Row " + std::to_string(m) + " of the local adjustment has " + std::to_string(w.size()) +
                                     " weights, the background has " + std::to_string(r.L) + ".");
        r.weights.insert(r.weights.end(), w.begin(), w.end());
        r.detail.insert(r.detail.end(), {e.detail.residualWeight, e.detail.gain, e.detail.sigma});
        if (!std::isfinite(e.saturation) || e.saturation < 0 || e.saturation > NLE_LOCAL_SATURATION_MAX)
            throw std::runtime_error("Row " + std::to_string(m) + " of the local adjustment: the saturation must be finite and in [0, " +
                                     std::to_string(NLE_LOCAL_SATURATION_MAX) + "].");
        r.saturation.push_back(e.saturation);
        r.chroma = r.chroma || e.saturation != 1;
        if (!std::isfinite(e.clipPercent) || e.clipPercent > 25 || !std::isfinite(e.equalise) || e.equalise < 0 || e.equalise > 1)
            throw std::runtime_error("Row " + std::to_string(m) + " of the local adjustment: clipPercent must be finite and at most 25 "
                                     "(negative: no levels), equalise finite and in [0, 1].");
        const bool hist = e.clipPercent >= 0 || e.equalise > 0, on = hist || !(e.shadows == 0 && e.highlights == 0);
        r.tone.insert(r.tone.end(), {e.shadows, e.highlights, e.clipPercent, e.equalise});
        r.histOn.push_back(hist ? 1 : 0);
        r.anyHist = r.anyHist || hist;
        r.curveOn.push_back(on ? 1 : 0);
        r.anyCurve = r.anyCurve || on;
        // (a row with a histogram gets its curve once the counts are known; the slopes are checked here either way)
        if (on) check(nle_tone_curve(nullptr, e.shadows, e.highlights, -1, 0, r.curves.data() + m * (NLE_TONE_KNOTS + 2)), nullptr);
    }
    return r;
}

const char kLocalOneDevice[] = "Local adjustments run on one device: this filter was trained on a device group (NLE_DEVICES).";

}  // namespace

Image NLEFilter::enhanceLocal(const Image& image, const std::vector<Image>& strokes, const std::vector<LocalEdit>& edits,
                              const LocalEdit& background, DType spread, DType floor) const {
    refuse_hdr(image, "enhanceLocal");
    if (image.channels() != 3 || (image.depth() != NLE_8U && image.depth() != NLE_16U))
        throw std::runtime_error("Can only enhance RGB image.");
    if (!group_.empty()) throw std::runtime_error(kLocalOneDevice);
    requireSize(image.total(), kTrainedSize);
    const int M = (int)strokes.size();
    if (M < 1 || M > NLE_REGION_MAX)
        throw std::runtime_error("Local adjustments take 1 to " + std::to_string(NLE_REGION_MAX) + " strokes.");
    if ((int)edits.size() != M) throw std::runtime_error("Local adjustments need one edit per stroke.");
    std::vector<const LocalEdit*> rows;
    for (const LocalEdit& e : edits) rows.push_back(&e);
    const LocalRowsHost r = local_rows(background, rows);
    const size_t np = image.total();
    // the stroke planes as 0 / 1 and their scales c_m = N / sum s_m, as enhanceRegions makes them
    std::vector<double> scale((size_t)M);
    std::vector<float> planes((size_t)M * np);
    for (int m = 0; m < M; ++m) {
        const Image& s = strokes[m];
        if (s.channels() != 1 || s.depth() != NLE_8U || s.rows != image.rows || s.cols != image.cols)
            throw std::runtime_error("Stroke " + std::to_string(m + 1) + " must be a one-channel 8-bit image of the image's size.");
        const unsigned char* b = s.ptr<unsigned char>();
        double sum = 0.0;
        for (size_t i = 0; i < np; ++i) {
            const float v = b[i] >= 128 ? 1.f : 0.f;
            planes[(size_t)m * np + i] = v;
            sum += v;
        }
        if (!(sum > 0)) throw std::runtime_error("Stroke " + std::to_string(m + 1) + " is empty (no byte >= 128).");
        scale[m] = (double)np / sum;
    }
    Dev d_s(ctx_, planes.size() * 4), d_q;  // d_q: the spreads, kept only for the chroma call
    if (r.chroma) d_q = Dev(ctx_, planes.size() * 4);
    check(nle_dev_upload(ctx_, d_s.p, planes.data(), planes.size() * 4), ctx_);
    const bool deep = is_deep(image);
    localLevels_.clear();
    std::vector<double> curves = r.curves;
    const auto op = [&](const float* d_x, float* d_y, float* d_a, float* d_b) {
        if (r.anyHist) {
            check(nle_apply_local_auto(f_, d_x, image.rows, image.cols, r.L, d_s.f(), M, scale.data(), spread, floor, r.weights.data(),
                                       r.detail.data(), r.tone.data(), deep ? NLE_REGION_OUT_F32 : NLE_REGION_OUT_ROUNDED8, d_y,
                                       r.chroma ? d_q.f() : nullptr, curves.data()), ctx_);
            localLevels_ = r.levels(curves.data());
        } else {
            check(nle_apply_local(f_, d_x, image.rows, image.cols, r.L, d_s.f(), M, scale.data(), spread, floor, r.weights.data(),
                                  r.detail.data(), r.anyCurve ? r.curveOn.data() : nullptr, r.anyCurve ? r.curves.data() : nullptr,
                                  deep ? NLE_REGION_OUT_F32 : NLE_REGION_OUT_ROUNDED8, d_y, r.chroma ? d_q.f() : nullptr), ctx_);
        }
        if (r.chroma)
            check(nle_local_chroma(ctx_, d_a, d_b, d_q.f(), M, (long long)np, (long long)np, r.saturation.data(), floor, d_a, d_b), ctx_);
    };
    return deep ? edit_deep_lab(ctx_, image, op) : edit_8bit_lab(ctx_, image, r.chroma, op);
}

Image NLEFilter::enhanceSegmentsLocal(const Image& image, const LocalEdit& background, const std::vector<LocalEdit>& edits) const {
    refuse_hdr(image, "enhanceSegmentsLocal");
    if (is_deep(image)) throw std::runtime_error("Segment edits take an 8-bit image: deep colour (16 bit) is built for enhance only.");
    if (image.channels() != 3 || image.depth() != NLE_8U) throw std::runtime_error("Can only enhance RGB image.");
    if (!group_.empty()) throw std::runtime_error(kLocalOneDevice);
    requireSize(image.total(), kTrainedSize);
    if (!segmentSpreads_) throw std::runtime_error("enhanceSegmentsLocal needs a segment() of this filter first.");
    const int C = segmentCount_;
    if ((int)edits.size() > C)
        throw std::runtime_error("Segment edits take at most one edit per segment (" + std::to_string(C) + ").");
    std::vector<const LocalEdit*> rows;
    for (int c = 0; c < C; ++c) rows.push_back(c < (int)edits.size() ? &edits[c] : &background);
    const LocalRowsHost r = local_rows(background, rows);
    const long long n = (long long)image.total();
    const float* d_q = static_cast<const float*>(segmentSpreads_.get());
    Dev d_layers(ctx_, (size_t)r.L * n * 4);
    localLevels_.clear();
    std::vector<double> curves = r.curves;
    return edit_8bit_lab(ctx_, image, r.chroma, [&](const float* d_x, float* d_y, float* d_a, float* d_b) {
        check(nle_apply_layers(f_, d_x, image.rows, image.cols, r.L, d_layers.f()), ctx_);
        if (r.anyHist) {  // the stage calls of nle_apply_local_auto, on the segments' spreads
            std::vector<long long> counts((size_t)(C + 1) * (NLE_TONE_BINS + 2));
            std::vector<double> scale((size_t)C + 1);
            for (int m = 0; m <= C; ++m) scale[m] = r.weights[(size_t)m * r.L + (r.L - 1)];
            check(nle_region_histograms(ctx_, d_layers.f() + (size_t)(r.L - 1) * n, d_q, C, n, n, scale.data(), r.histOn.data(),
                                        segmentFloor_, counts.data()), ctx_);
            for (int m = 0; m <= C; ++m) {
                if (!r.histOn[m]) continue;
                const long long* row = counts.data() + (size_t)m * (NLE_TONE_BINS + 2);
                const long long mass = std::accumulate(row, row + NLE_TONE_BINS + 2, 0ll);
                const double* tn = r.tone.data() + 4 * m;
                // (less than one pixel's mass: the curve of the two slopes alone, which local_rows has made)
                if (mass >= NLE_REGION_WEIGHT_ONE)
                    check(nle_tone_curve(row, tn[0], tn[1], tn[2], tn[3], curves.data() + (size_t)m * (NLE_TONE_KNOTS + 2)), nullptr);
            }
            localLevels_ = r.levels(curves.data());
        }
        check(nle_local_combine(ctx_, d_x, d_layers.f(), r.L, d_q, C, n, n, n, r.weights.data(), r.detail.data(),
                                r.anyCurve ? r.curveOn.data() : nullptr, r.anyCurve ? curves.data() : nullptr, segmentFloor_,
                                NLE_REGION_OUT_ROUNDED8, d_y), ctx_);
        if (r.chroma) check(nle_local_chroma(ctx_, d_a, d_b, d_q, C, n, n, r.saturation.data(), segmentFloor_, d_a, d_b), ctx_);
    });
}

NLEFilter::Residual NLEFilter::nystromResidual(const Image& image, int nRowSamples, int nColSamples, DType hx, DType hy, int form,
                                               double thresh) const {
    refuse_hdr(image, "nystromResidual");
    if (exact) throw std::runtime_error("nystromResidual: the exact filter has no Nystrom extension");
    const bool bgr = image.channels() == 3 && image.depth() == NLE_8U, deep = is_deep(image);
    if (!bgr && !deep && !(image.channels() == 1 && image.depth() == NLE_64F))
        throw std::runtime_error("nystromResidual takes a 1-channel CV_64F plane or a 3-channel 8-bit or 16-bit image");
    if (nRowSamples > image.rows || nColSamples > image.cols) throw std::runtime_error(kSampleCount);
    nle_ctx* c = shared_ctx();
    const size_t n = image.total();
    LabPlanes in;
    if (bgr) {
        in = lab_planes(c, image.ptr<unsigned char>(), n, true, chromaBandwidth != 0);  // as trainForEnhancement
    } else if (deep) {  // as trainForEnhancement on a 16-bit image: the guide, and the rounded a and b
        Lab16Planes in16 = lab16_planes(c, image, chromaBandwidth != 0, true);
        DeepChroma ab = deep_chroma_planes(c, in16, n, chromaBandwidth != 0);
        in.L = std::move(in16.guide);
        in.a = std::move(ab.a);
        in.b = std::move(ab.b);
    } else {
        in.L = upload_plane(c, image);
    }
    Dev d_r(c, n * 4);
    double s[4] = {0, 0, 0, 0};
    {  // the shared ctx's options as a train sets them
        TrainOptions options(c, *this, in.a.f(), in.b.f());
        check(nle_nystrom_residual(c, in.L.f(), image.rows, image.cols, nRowSamples, nColSamples, hx, hy, form, thresh, d_r.f(), s),
              c);
    }
    std::vector<float> h(n);
    check(nle_dev_download(c, h.data(), d_r.p, n * 4), c);
    Residual out;
    out.map = image_f64(h.data(), image.rows, image.cols);
    out.sum = s[0], out.max = s[1], out.argmax = (long long)s[2], out.count = (long long)s[3];
    return out;
}

Vec NLEFilter::eigvals() const {
    if (!f_) return Vec();
    Vec v(K());
    nle_filter_eigvals(f_, v.data());
    return v;
}

Mat NLEFilter::eigvecs() const {
    if (!f_) return Mat();
    const long long n = n_local();
    const int nK = K();
    const float* d_V = nullptr;
    int ld = 0;
    nle_filter_eigvecs(f_, &d_V, &ld);
    std::vector<float> h((size_t)n * ld);
    check(nle_dev_download(ctx_, h.data(), d_V, h.size() * 4), ctx_);
    Mat V((int)n, nK);
    for (int k = 0; k < nK; ++k)
        for (long long i = 0; i < n; ++i) V((int)i, k) = h[(size_t)i * ld + k];
    return V;
}

void NLEFilter::timings(double ms[6]) const {
    if (f_) nle_filter_timings(f_, ms);
}

std::vector<long long> NLEFilter::samplePixels() const {
    int p = 0;
    if (!f_ || nle_filter_sample_pixels(f_, nullptr, &p) != NLE_OK) return {};
    std::vector<long long> idx((size_t)p);
    nle_filter_sample_pixels(f_, idx.data(), &p);
    return idx;
}

void NLEFilter::diag(int info[8]) const {
    std::fill(info, info + 8, 0);
    if (f_) nle_filter_diag(f_, info);
}

}  // namespace nle
