// nle/filter.hpp -- C++ drop-in surface of the MI355X-native nonlocal filter.
//
// Same names, parameter order, defaults, return-tuple order and exceptions as the reference's
// include/filter.hpp:10-54 (lightalchemist/nonlocal-image-edit).  The reference's types come
// from Eigen and OpenCV, neither of which exists in this build; the types below are minimal
// stand-ins with the SAME memory layouts (column-major fp64 matrix = Eigen::MatrixXd, row-major
// image = continuous cv::Mat), so a build that has Eigen/OpenCV can map them without copies.
// Every function here is a thin host wrapper over the C ABI in include/nle.h (libnle_hip.so);
// all N-sized arithmetic runs in HIP kernels on the GPU, there is no CPU fallback.
#pragma once
#ifndef NLE_FILTER_HPP
#define NLE_FILTER_HPP

#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <tuple>
#include <utility>
#include <vector>

struct nle_ctx;
struct nle_filter;

namespace nle {

using DType = double;      // include/filter.hpp:12
const double EPS = 1e-10;  // include/filter.hpp:14

struct Point {  // include/filter.hpp:15-18
    int row;
    int col;
};

// Eigen::VectorXd stand-in
class Vec {
public:
    Vec() = default;
    explicit Vec(int n, double v = 0.0) : d_((size_t)n, v) {}
    Vec(std::initializer_list<double> l) : d_(l) {}
    static Vec Ones(int n) { return Vec(n, 1.0); }
    int size() const { return (int)d_.size(); }
    int rows() const { return (int)d_.size(); }
    int cols() const { return 1; }
    double& operator()(int i) { return d_[(size_t)i]; }
    double operator()(int i) const { return d_[(size_t)i]; }
    double* data() { return d_.data(); }
    const double* data() const { return d_.data(); }
    Vec head(int n) const {
        Vec v(n);
        for (int i = 0; i < n; ++i) v(i) = d_[(size_t)i];
        return v;
    }

private:
    std::vector<double> d_;
};

// Eigen::MatrixXd stand-in: COLUMN-major, fp64
class Mat {
public:
    Mat() = default;
    Mat(int r, int c, double v = 0.0) : r_(r), c_(c), d_((size_t)r * c, v) {}
    static Mat Identity(int r, int c) {
        Mat m(r, c);
        for (int i = 0; i < r && i < c; ++i) m(i, i) = 1.0;
        return m;
    }
    int rows() const { return r_; }
    int cols() const { return c_; }
    double& operator()(int i, int j) { return d_[(size_t)j * r_ + i]; }
    double operator()(int i, int j) const { return d_[(size_t)j * r_ + i]; }
    double* data() { return d_.data(); }
    const double* data() const { return d_.data(); }
    Mat transpose() const {
        Mat t(c_, r_);
        for (int j = 0; j < c_; ++j)
            for (int i = 0; i < r_; ++i) t(j, i) = (*this)(i, j);
        return t;
    }
    Mat leftCols(int n) const {
        Mat m(r_, n);
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < r_; ++i) m(i, j) = (*this)(i, j);
        return m;
    }

private:
    int r_ = 0, c_ = 0;
    std::vector<double> d_;
};

Mat operator*(const Mat& a, const Mat& b);  // small host products (tests, glue)

// Eigen::PermutationMatrix stand-in: indices()[i] = row-major pixel index of the i-th pixel in the
// reference's [selected; rest] order (src/filter.cpp:156-164)
struct Permutation {
    std::vector<int> idx;
    std::vector<int>& indices() { return idx; }
    const std::vector<int>& indices() const { return idx; }
    int size() const { return (int)idx.size(); }
};

// continuous cv::Mat stand-in: ROW-major, interleaved channels; depth CV_8U, CV_16U (deep-colour images: imread16,
// trainForEnhancement, enhance), CV_32F (linear-light HDR images: imreadHDR, trainForToneMapping, toneMap) or CV_64F
enum { NLE_8U = 0, NLE_16U = 2, NLE_32F = 5, NLE_64F = 6 };
const int OPENCV_MAT_TYPE = NLE_64F;  // include/filter.hpp:13
class Image {
public:
    int rows = 0, cols = 0;
    Image() = default;
    Image(int r, int c, int depth, int channels = 1)
        : rows(r), cols(c), depth_(depth), ch_(channels),
          buf_((size_t)r * c * channels * (depth == NLE_64F ? 8 : depth == NLE_32F ? 4 : depth == NLE_16U ? 2 : 1)) {}
    int channels() const { return ch_; }
    int depth() const { return depth_; }
    size_t total() const { return (size_t)rows * cols; }
    bool empty() const { return rows == 0 || cols == 0; }
    template <typename T>
    T* ptr(int r = 0) {
        return reinterpret_cast<T*>(buf_.data()) + (size_t)r * cols * ch_;
    }
    template <typename T>
    const T* ptr(int r = 0) const {
        return reinterpret_cast<const T*>(buf_.data()) + (size_t)r * cols * ch_;
    }
    template <typename T>
    T& at(int r, int c) {
        return ptr<T>(r)[c];
    }
    template <typename T>
    const T& at(int r, int c) const {
        return ptr<T>(r)[c];
    }
    Image clone() const { return *this; }

private:
    int depth_ = NLE_8U, ch_ = 1;
    std::vector<unsigned char> buf_;
};

// include/utils.hpp:11-41
inline int to1DIndex(int row, int col, int ncols) { return row * ncols + col; }
inline std::pair<int, int> to2DCoords(int index, int ncols) { return std::make_pair(index / ncols, index % ncols); }
Image eigen2opencv(const Vec& v, int nrows, int ncols);
Vec opencv2eigen(const Image& mat);

// ---- the five free functions, include/filter.hpp:20-33 ----
std::tuple<Permutation, Mat, Mat> computeKernel(const Image& mat, int nRowSamples, int nColSamples, DType hx,
                                                DType hy);
std::pair<Mat, Vec> eigenDecomposition(const Mat& M, DType eps = EPS);
std::pair<Vec, Mat> nystromApproximation(const Mat& Ka, const Mat& Kab);
std::pair<Mat, Mat> sinkhorn(const Mat& phi, const Vec& eigvals, int maxIter = 10);
std::pair<Mat, Vec> orthogonalize(const Mat& Wa, const Mat& Wab, int nEigVectors = 5, DType eps = EPS);

// src/filter.cpp:334-347 (a global in the reference, not declared in its header)
Vec transformEigenValues(const Vec& eigvals, const std::vector<DType>& weights);

// 8-bit BGR <-> Lab as cv::cvtColor(COLOR_BGR2Lab / COLOR_Lab2BGR) documents it (host)
Image bgr2lab8(const Image& bgr);
Image lab2bgr8(const Image& lab);
// the same on the GPU (what NLEFilter uses); agree with the host forms except for isolated rounding ties
Image bgr2lab8_device(const Image& bgr);
Image lab2bgr8_device(const Image& lab);

// cv::bilateralFilter(src, dst, -1, sigmaColor, sigmaSpace, BORDER_DEFAULT) on one 8-bit channel, as the denoise
// wrapper calls it (src/filter.cpp:371,535): host form and device form (bit-identical: same fp32 tables, same
// summation order); see nle_bilateral8 in nle.h for what "as OpenCV documents it" covers
Image bilateralFilter8(const Image& plane, double sigmaColor, double sigmaSpace);
Image bilateralFilter8_device(const Image& plane, double sigmaColor, double sigmaSpace);

// the options of NLEFilter::enhance / toneMap with the out-of-span detail layer and the detail curve (new here; see there)
struct DetailOptions {
    double residualWeight = 0, gain = 1, sigma = 0;
    bool active() const { return !(residualWeight == 0 && (sigma == 0 || gain == 1)); }
};

// the options of NLEFilter::enhance with the base tone curve (new here; see there)
struct ToneOptions {
    double shadows = 0, highlights = 0, clipPercent = -1, equalise = 0;
    bool active() const { return !(shadows == 0 && highlights == 0 && clipPercent < 0 && equalise == 0); }
};
// the range [lo, hi] the last enhance with active ToneOptions laid its curve over (0, 255 without auto levels)
struct ToneLevels {
    double lo = 0, hi = 255;
    bool valid = false;
};

// one row of NLEFilter::enhanceLocal / enhanceSegmentsLocal (new here; see there): the whole edit of a region, or of the
// background -- layer weights (empty: the background's), the detail options, the two slopes of a base tone curve of its own
// (both 0: no curve) and the saturation of a and b (1: untouched); clipPercent >= 0 (auto levels) and equalise > 0 lay that
// curve over the row's own membership-weighted histogram of the base layer (nle_region_histograms in nle.h), as
// ToneOptions has them for the whole image
struct LocalEdit {
    std::vector<DType> weights;
    DetailOptions detail;
    DType shadows = 0, highlights = 0, saturation = 1;
    DType clipPercent = -1, equalise = 0;
};

// the options of NLEFilter::segment (new here; see there): the number of segments, how far a segment's indicator spreads
// (the t of G = V lambda^t V^T), the cap on the iterations, and the membership floor enhanceSegments combines with
struct SegmentOptions {
    int count = 0;
    double spread = 4;
    int maxIterations = 40;
    double floor = 0.05;
};
// what the last NLEFilter::segment found: per segment its pixels and their mean L on the plane the filter was trained on
// (0 for an empty segment), the iterations made, whether the last one changed no label, and its objective
struct SegmentReport {
    std::vector<long long> counts;
    std::vector<double> meanL;
    int iterations = 0;
    bool converged = false;
    double objective = 0;
    bool valid = false;
};

// the options of NLEFilter::trainForDenoise / denoise for the MSE-guided denoiser (new here; DESIGN.md section 3.16, the
// arithmetic is stated in nle.h at nle_nlm8).  The two choices are independent; the defaults are the reference's flow.
//   prefilter   NLE_PREFILTER_BILATERAL (0): cv::bilateralFilter as the reference calls it; NLE_PREFILTER_NLM (1): wherever
//               that flow calls the bilateral filter -- the plane the filter is trained on, the L that replaces the image's --
//               nle_nlm8 runs instead, with sigma = noiseSigma or nle_plane_noise of the plane being filtered and P, S, h from
//               the table for grey images of Buades, Coll & Morel, "Non-Local Means Denoising", IPOL 2011, cut to the kernel's
//               limits: sigma <= 15: P 1, S 10, h 0.40 sigma; <= 30: P 2, S 10, h 0.40 sigma; above: P 3, S 10, h 0.35 sigma
//               (taken from the literature, not tuned here).  nlmH > 0 replaces h; h == 0 (sigma == 0): the plane is copied.
//               sigmaColor and sigmaSpace are then unused.
//   glide       denoise shrinks every plane, L included, by mu^k with k chosen per plane by nle_mse_shrink: sigma per plane
//               (given or estimated), all three noisy planes pre-filtered, the coefficients V^T of the pre-filtered planes
//               standing in for the clean signal's, k searched on [0, the call's shrink factor] in 256 steps; then the filter
//               runs on the NOISY planes.  Needs a filter trained by trainForDenoise.
//   noiseSigma  >= 0: the noise level of every plane; < 0: estimated per plane (an upper estimate, see nle_plane_noise)
// One device (a filter trained on a device group throws); 8-bit images only.
struct DenoiseOptions {
    int prefilter = 0;  // NLE_PREFILTER_BILATERAL
    bool glide = false;
    double noiseSigma = -1;
    double nlmH = 0;
};
// what the last denoise with DenoiseOptions::glide chose for L, a and b: the noise level used, the power k and MSE(k)
struct DenoiseReport {
    double sigma[3] = {0, 0, 0}, k[3] = {0, 0, 0}, mse[3] = {0, 0, 0};
    bool valid = false;
};

// include/filter.hpp:35-54.  The trained state (m_eigvecs N x K', m_eigvals) lives on the GPU.
class NLEFilter {
public:
    // copyable like the reference's class (its state is two Eigen members, include/filter.hpp:52-53): copies
    // share the trained, immutable device-side filter
    NLEFilter();
    ~NLEFilter();

    void trainForEnhancement(const Image& image, int nRowSamples, int nColSamples, DType hx, DType hy,
                             int nSinkhornIter = 10, int nEigenVectors = 5);
    Image enhance(const Image& I, const std::vector<DType>& weights) const;
    // Deep colour (new here): both also take a 16UC3 image (imread16).  The train converts 16-bit
    // sRGB to float Lab on the device and runs on the guide, L rounded to the 256 levels of the 8-bit path (patchRadius,
    // sampler, exact and chromaBandwidth apply as they do there; chroma takes a and b rounded the same way); enhance applies
    // the filter to the unrounded L and returns a 16UC3 image: nothing is rounded to 8 bits.  One device; enhanceRegions,
    // trainForDenoise and denoise throw for a 16-bit image.
    // HDR tone mapping (new here; DESIGN.md section 3.14, the arithmetic is stated in nle.h at nle_hdr_range): a 32FC3
    // linear-light BGR image (imreadHDR).  The train finds the image's luminance range on the device, writes log-luminance
    // on the scale of an 8-bit L plane and trains on its 256-level guide (patchRadius, sampler and exact apply as for
    // enhance); it keeps the range in the filter.  toneMap applies the filter to the unrounded log-luminance of `I` with the
    // trained range -- the last weight multiplies the base layer, so one below 1 compresses the large-scale variation and
    // keeps the detail -- and returns a 16UC3 sRGB image; saturation in (0, 2] is the exponent of the colour ratios.  One
    // device; both throw with a non-zero chromaBandwidth, and the 8- and 16-bit methods throw for a 32F image.
    void trainForToneMapping(const Image& image, int nRowSamples, int nColSamples, DType hx, DType hy,
                             int nSinkhornIter = 10, int nEigenVectors = 5);
    Image toneMap(const Image& I, const std::vector<DType>& weights, DType saturation = 1) const;
    // The out-of-span detail layer and the detail curve (new here; DESIGN.md section 3.15, nle_detail_combine in nle.h states
    // the rule).  The layers that `weights` scale sum to V V^T x, not to x: what of the plane the trained eigenvectors do not
    // span is in no layer.  residualWeight gives that residual back as one more layer (1: weights of all ones return the
    // plane), and gain in [0, 3] with sigma > 0 sends the residual and every layer but the base through a monotone curve of
    // slope `gain` at 0 that tends to the identity for amplitudes far above sigma -- texture is boosted (or cored, gain < 1)
    // and edges keep their size.  Options with residualWeight == 0 and (sigma == 0 or gain == 1) are inactive: the call is
    // the plain method's, bit for bit.  Active options run nle_apply_detail on the plane the plain method filters (8 bit:
    // rounded to levels; 16 bit: the unrounded L; 32F: the unrounded log-luminance, the last weight still the base weight).
    // One device: a filter trained on a device group throws; 1 to NLE_REGION_LAYERS_MAX weights.
    Image enhance(const Image& I, const std::vector<DType>& weights, const DetailOptions& detail) const;
    Image toneMap(const Image& I, const std::vector<DType>& weights, DType saturation, const DetailOptions& detail) const;
    // The base tone curve (new here; DESIGN.md section 3.18, nle_tone_combine in nle.h states the rule): the weighted base
    // layer -- the one plane the detail options never remap -- passes a monotone curve before the layers are summed.
    // shadows and highlights in [-1, 1] change the curve's slope at its dark and its bright end to 1 + shadows and
    // 1 + highlights; clipPercent in [0, 25] lays the curve over the range that remains when that share of the base
    // layer's pixels is clipped at either end (auto levels; < 0: the range [0, 255]); equalise in [0, 1] blends the curve
    // with the equalisation of the base layer's histogram inside that range.  The detail layers pass unchanged: no halo.
    // Inactive options (all four at their defaults) are the method above, bit for bit.  Active options run nle_apply_tone
    // on the plane that method filters, for 8-bit and 16-bit images.  One device: a filter trained on a device group
    // throws; 1 to NLE_REGION_LAYERS_MAX weights.  lastToneCurve(): the range of the last such call.
    Image enhance(const Image& I, const std::vector<DType>& weights, const DetailOptions& detail, const ToneOptions& tone) const;
    ToneLevels lastToneCurve() const { return toneLevels_; }
    // region edits (new here; nle_apply_regions in nle.h states the rule): enhance with layer weights of its own for every
    // scribbled region.  strokes[m]: a one-channel 8-bit image of I's size, a pixel belongs to the stroke where its byte is
    // >= 128; regionWeights[m]: the weights of region m, as many as `weights`, which is the background's row.  Each stroke
    // is spread along the trained affinity (V lambda^spread V^T s, scaled to mean 1) and the spreads decide, pixel by
    // pixel, how the rows blend; below `floor` of total influence a pixel blends to the background.  The defaults are the
    // values of the two CPU experiments behind the definition, not tuned further.  Throws
    // std::runtime_error for an all-zero stroke, a size mismatch, a weight count other than weights.size(), more than
    // NLE_REGION_MAX strokes or NLE_REGION_LAYERS_MAX weights, and for a filter trained on a device group (NLE_DEVICES).
    Image enhanceRegions(const Image& I, const std::vector<Image>& strokes,
                         const std::vector<std::vector<DType>>& regionWeights, const std::vector<DType>& weights,
                         DType spread = 4, DType floor = 0.05) const;
    // automatic regions (new here; nle_filter_segment in nle.h states the rule): the regions a
    // region edit needs, proposed by the trained filter itself instead of hand-drawn strokes -- kernel k-means of the pixels
    // on the affinity V lambda^spread V^T, from equal-population cuts of the plane the filter was trained on; nothing is
    // random, so two calls give the same labels.  segment needs a filter trained by trainForEnhancement on one device with
    // keepTrainPlane set (see there); it returns the labels as an 8UC1 image and keeps the segments' spreads on the device.
    // enhanceSegments is enhanceRegions with those spreads as the memberships and options.floor as the floor: `weights` is
    // the background's row, segmentWeights[c] the row of segment c -- `weights` again where it is empty or missing; 8-bit
    // images.  Both throw std::runtime_error for a count outside 1 .. NLE_REGION_MAX, whatever nle_filter_segment refuses,
    // a filter trained on a device group, and enhanceSegments without a segment() since the last train.
    Image segment(const SegmentOptions& options);
    SegmentReport lastSegments() const { return segmentReport_; }
    Image enhanceSegments(const Image& I, const std::vector<DType>& weights,
                          const std::vector<std::vector<DType>>& segmentWeights) const;
    // local adjustments (new here; nle_local_combine in nle.h states the rule): every region gets the
    // whole edit of its own -- its layer weights, residual weight and detail curve, a base tone curve from its shadows and
    // highlights (nle_tone_curve(NULL, shadows, highlights, -1, 0), switched on where one of the two is non-zero) and the
    // saturation of a and b about 128 -- and the memberships of the region edits blend the rows' results, pixel by pixel.
    // enhanceLocal: strokes, spread and floor as enhanceRegions takes them, edits[m] the row of strokes[m], `background` row 0
    // (its weights give the layer count); 8-bit and 16-bit images (the latter on the unrounded L, a and b).
    // enhanceSegmentsLocal: the same on the spreads and floor of the last segment(), like enhanceSegments: edits[c] is the row
    // of segment c, the background's where it is missing; 8-bit images.  An edit with empty weights takes the background's.
    // With every saturation 1 the chroma planes are not touched.  Both throw std::runtime_error for an HDR image, a filter
    // trained on a device group, counts out of range, a weight count other than the background's, a saturation outside
    // [0, NLE_LOCAL_SATURATION_MAX] and whatever nle_apply_local / nle_local_combine / nle_tone_curve refuse.
    // Per-region auto levels and equalise (new here): exactly when some row has clipPercent >= 0 or
    // equalise > 0, the rows' curves come from nle_region_histograms -- enhanceLocal is then nle_apply_local_auto,
    // enhanceSegmentsLocal the same stage calls on the segments' spreads; otherwise both make the calls they made.
    // lastLocalLevels(): one entry per row of the last such call (row 0 the background), valid where the row had either.
    Image enhanceLocal(const Image& I, const std::vector<Image>& strokes, const std::vector<LocalEdit>& edits,
                       const LocalEdit& background, DType spread = 4, DType floor = 0.05) const;
    Image enhanceSegmentsLocal(const Image& I, const LocalEdit& background, const std::vector<LocalEdit>& edits) const;
    std::vector<ToneLevels> lastLocalLevels() const { return localLevels_; }
    // include/filter.hpp:40-45: the filter is trained on the bilateral-filtered L channel; denoise shrinks the
    // eigenvalues to min(lambda, 1)^k on the a and b channels (src/filter.cpp:349-410, 521-538)
    void trainForDenoise(const Image& image, int nRowSamples, int nColSamples, DType hx, DType hy, int nSinkhornIter,
                         int nEigenVectors, int sigmaColor = 10, int sigmaSpace = 10);
    Image denoise(const Image& I, DType k, int sigmaColor = 10, int sigmaSpace = 10) const;
    // the same with DenoiseOptions (new here, see there); default options are the two methods above, byte for byte
    void trainForDenoise(const Image& image, int nRowSamples, int nColSamples, DType hx, DType hy, int nSinkhornIter,
                         int nEigenVectors, int sigmaColor, int sigmaSpace, const DenoiseOptions& options);
    Image denoise(const Image& I, DType k, int sigmaColor, int sigmaSpace, const DenoiseOptions& options) const;
    DenoiseReport lastDenoiseReport() const { return denoiseReport_; }

    // private in the reference (include/filter.hpp:47-50); public here so tests and other hosts can
    // drive the hot path on a luminance plane directly
    Image apply(const Image& channel, const Vec& transformedEigVals) const;
    void trainFilter(const Image& channel, int nRowSamples, int nColSamples, DType hx, DType hy, int nSinkhornIter,
                     int nEigenVectors);
    // train on an fp32 luminance plane that is already on the device
    // (d_a, d_b: the a and b planes for chromaBandwidth > 0, as nle_ctx_set_chroma takes them; both null: no chroma)
    void trainOnDevice(const float* d_lum, int rows, int cols, int nRowSamples, int nColSamples, DType hx, DType hy,
                       int nSinkhornIter, int nEigenVectors, const float* d_a = nullptr, const float* d_b = nullptr);
    // per-layer outputs (L planes, CV_64F) -- what the 1e-4 per-detail-layer bar compares
    std::vector<Image> applyLayers(const Image& channel, int nLayers) const;
    // several planes through the filter in one call (nle_apply_planes): responses[m] are the transformed eigenvalue
    // vectors of channels[m] (one or more each); returns one CV_64F plane per response, those of channel 0 first, each bit
    // for bit what apply(channels[m], responses[m][l]) returns.  Host buffers in and out, like apply.
    std::vector<Image> applyPlanes(const std::vector<Image>& channels, const std::vector<std::vector<Vec>>& responses) const;

    // The Nystrom residual map of a sample grid and bandwidths on this image (nle_nystrom_residual in nle.h; new here): r_i =
    // 1 - k_i^T pinv(K_A) k_i per pixel, the diagonal of K - K~ for the extension a train with the same arguments uses -- where
    // the samples fail to explain a pixel.  `image`: a 1-channel CV_64F luminance plane (as trainFilter takes it) or a
    // 3-channel 8-bit BGR image (as trainForEnhancement takes it: its L channel, and its a and b planes when chromaBandwidth
    // is set).  Uses patchRadius, sampler and chromaBandwidth like a train -- a bare plane has no a and b planes, so
    // chromaBandwidth is ignored for it, as trainFilter ignores it; needs no trained filter and leaves one untouched.
    // One device (not NLE_DEVICES groups); throws std::runtime_error with `exact` set (that filter has no extension) and for
    // whatever the call refuses.  form: NLE_RESID_AUTO / _ROWS / _FUSED.
    struct Residual {
        Image map;                // CV_64F, the fp32 values of the device map
        double sum = 0, max = 0;  // sum_i r_i (the trace-norm error of the extension), max_i r_i
        long long argmax = 0;     // row-major index of the first maximum
        long long count = 0;      // pixels with r_i > thresh
    };
    Residual nystromResidual(const Image& image, int nRowSamples, int nColSamples, DType hx, DType hy, int form = 0,
                             double thresh = 0.5) const;

    Vec eigvals() const;                 // m_eigvals
    Mat eigvecs() const;                 // m_eigvecs, downloaded (N x K')
    void timings(double ms[6]) const;    // nle_filter_timings
    std::vector<long long> samplePixels() const;  // nle_filter_sample_pixels: the set trained on, row-major, ascending
    // nle_filter_diag: {formulation, p, rank Ka, rank Wa, rank Q, K', chol(Ka), chol(Wa)}
    void diag(int info[8]) const;
    bool verbose = true;                 // the reference's stdout stage banners (:483-498,506)
    // patch (non-local-means) affinities over (2 patchRadius + 1)^2 neighbourhoods for trainForEnhancement /
    // trainForDenoise / trainFilter (nle_ctx_set_patch_radius; new here, 0 = the reference's single-value affinity)
    int patchRadius = 0;
    // sample selection for trainForEnhancement / trainForDenoise / trainFilter (nle_ctx_set_sampler; new here,
    // NLE_SAMPLER_GRID = the reference's grid, NLE_SAMPLER_FARTHEST = farthest-point selection, NLE_SAMPLER_RESIDUAL (3) =
    // residual-greedy selection: pivoted Cholesky on the affinity)
    int sampler = 0;
    // the exact (Nystrom-free) filter for trainForEnhancement / trainForDenoise / trainFilter (NLE_MODE_EXACT_F64 around
    // the train; new here): one device, at most NLE_EXACT_MAX_PIXELS pixels, patchRadius 0 and the grid sampler
    bool exact = false;
    // chroma-aware (Lab) affinities for trainForEnhancement (nle_ctx_set_chroma; new here, 0 = the reference's
    // luminance-only affinity): the chroma bandwidth hc > 0, a chroma difference per pixel in the unit of hy.  Needs
    // patchRadius <= NLE_CHROMA_PATCH_RADIUS_MAX and not `exact`.  trainFilter takes a bare luminance plane, has no
    // chroma and ignores it; trainForDenoise throws if it is set (a and b are what that path estimates)
    double chromaBandwidth = 0;
    // trainForEnhancement on one device leaves its fp32 L plane on the device for segment() to start from (new here; 4 bytes
    // per pixel for the life of the filter, so only on request)
    bool keepTrainPlane = false;

private:
    nle_ctx* ctx_ = nullptr;
    std::shared_ptr<nle_filter> fh_;  // nle_filter_destroy when the last copy goes
    nle_filter* f_ = nullptr;         // == fh_.get()
    int rows_ = 0, cols_ = 0;
    bool denoiseTrained_ = false;            // the filter in hand came from trainForDenoise (what glide needs)
    mutable ToneLevels toneLevels_;          // enhance with active ToneOptions
    mutable std::vector<ToneLevels> localLevels_;  // enhanceLocal / enhanceSegmentsLocal: one per row
    mutable DenoiseReport denoiseReport_;    // denoise with DenoiseOptions::glide
    // segment(): the plane trainForEnhancement trained on (fp32, on the device; keepTrainPlane), the spreads of the last segmentation
    // (count planes) with its floor, and what it found
    std::shared_ptr<void> trainPlane_, segmentSpreads_;
    int segmentCount_ = 0;
    double segmentFloor_ = 0.05;
    SegmentReport segmentReport_;
    double hdrHi_ = 0, hdrRange_ = 0;  // trainForToneMapping: log2 of the largest luminance and the range in stops (0: none)
    // NLE_DEVICES=<dev>,<dev>,...: trainForEnhancement / enhance shard the image by row slabs over one context (and
    // one host thread per call) per listed device; rank r's filter is group_[r] and f_ == group_[0].get()
    std::vector<std::shared_ptr<nle_filter>> group_;
    long long n_local() const;  // pixels f_ holds (a rank's rows under a group); 0 when untrained
    int K() const;              // eigenvectors kept; 0 when untrained
    // throws `message` unless a trained filter holds exactly `pixels` pixels
    void requireSize(size_t pixels, const char* message) const;
    // a train starts on ctx c: the old filter goes, the reference's stage banners are printed
    void beginTrain(nle_ctx* c);
    // a train ended: fs (one filter, or one per rank of the group, on ctxs) become the state; the Eigvec lines
    void adopt(const std::vector<nle_ctx*>& ctxs, const std::vector<nle_filter*>& fs, int rows, int cols, int nEigenVectors);
};

}  // namespace nle

#endif
