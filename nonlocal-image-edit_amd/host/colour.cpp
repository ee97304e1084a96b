// The colour wrapper either side of the filter, host and device forms (include/nle/filter.hpp): 8-bit BGR <-> Lab as
// cv::cvtColor does it (bgr2lab8, lab2bgr8) and cv::bilateralFilter on one 8-bit channel (bilateralFilter8).  The host
// forms restate the integer / fp32 table algorithms (tables from the C ABI); the _device forms run csrc/colour.hip.
#include <algorithm>
#include <cmath>

#include "surface_internal.hpp"

namespace nle {

using namespace surface;

// ------------------------------------------------------------------ colour wrapper (host)
// cv::cvtColor on 8-bit images: both directions are OpenCV's integer table algorithms (tables from the C ABI)
Image bgr2lab8(const Image& bgr) {
    if (bgr.channels() != 3 || bgr.depth() != NLE_8U) throw std::runtime_error("bgr2lab8: 8UC3 image expected");
    // OpenCV's fixed-point 8-bit path (imgproc RGB2Lab_b; include/nle.h at nle_lab8_tables): exact integers
    unsigned short gam[256], cb[3072];
    int k[9];
    if (nle_lab8_tables(gam, cb, k) != NLE_OK) throw std::runtime_error("bgr2lab8: tables");
    auto sat = [](int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); };
    Image lab(bgr.rows, bgr.cols, NLE_8U, 3);
    const unsigned char* s = bgr.ptr<unsigned char>();
    unsigned char* d = lab.ptr<unsigned char>();
    for (size_t i = 0; i < bgr.total(); ++i, s += 3, d += 3) {
        const int B = gam[s[0]], G = gam[s[1]], R = gam[s[2]];
        const int fX = cb[(R * k[0] + G * k[1] + B * k[2] + 2048) >> 12];
        const int fY = cb[(R * k[3] + G * k[4] + B * k[5] + 2048) >> 12];
        const int fZ = cb[(R * k[6] + G * k[7] + B * k[8] + 2048) >> 12];
        d[0] = sat((296 * fY - 1336934 + 16384) >> 15);
        d[1] = sat((500 * (fX - fY) + 128 * 32768 + 16384) >> 15);
        d[2] = sat((200 * (fY - fZ) + 128 * 32768 + 16384) >> 15);
    }
    return lab;
}

Image lab2bgr8(const Image& lab) {
    if (lab.channels() != 3 || lab.depth() != NLE_8U) throw std::runtime_error("lab2bgr8: 8UC3 image expected");
    // OpenCV's integer 8-bit path (imgproc Lab2RGBinteger; include/nle.h at nle_lab8_inverse_tables): exact integers
    static std::vector<int> ab(36864);
    static unsigned short yf[512], ig[4096];
    static int k[9];
    static const bool ok = nle_lab8_inverse_tables(yf, ab.data(), ig, k) == NLE_OK;
    if (!ok) throw std::runtime_error("lab2bgr8: tables");
    Image bgr(lab.rows, lab.cols, NLE_8U, 3);
    const unsigned char* s = lab.ptr<unsigned char>();
    unsigned char* d = bgr.ptr<unsigned char>();
    auto enc = [&](const int* c, int x, int y, int z) {
        const int v = (c[0] * x + c[1] * y + c[2] * z + (1 << 13)) >> 14;
        return (unsigned char)ig[std::min(4095, std::max(0, v))];
    };
    for (size_t i = 0; i < lab.total(); ++i, s += 3, d += 3) {
        const int y = yf[2 * s[0]], fy = yf[2 * s[0] + 1];
        const int x = ab[fy + (((5 * s[1] * 53687 + (1 << 7)) >> 13) - 4194) + 8145];
        const int z = ab[fy - (((s[2] * 41943 + (1 << 4)) >> 9) - 10484) + 8145];
        d[0] = enc(k + 6, x, y, z);
        d[1] = enc(k + 3, x, y, z);
        d[2] = enc(k, x, y, z);
    }
    return bgr;
}

// the same conversions on the GPU (csrc/colour.hip) -- what NLEFilter uses; bit-identical to the host functions above
Image bgr2lab8_device(const Image& bgr) {
    if (bgr.channels() != 3 || bgr.depth() != NLE_8U) throw std::runtime_error("bgr2lab8: 8UC3 image expected");
    nle_ctx* c = shared_ctx();
    const size_t n = bgr.total();
    Dev d_in(c, n * 3), d_out(c, n * 3);
    check(nle_dev_upload(c, d_in.p, bgr.ptr<unsigned char>(), n * 3), c);
    check(nle_bgr2lab8(c, d_in.u8(), (long long)n, d_out.u8(), nullptr), c);
    Image lab(bgr.rows, bgr.cols, NLE_8U, 3);
    check(nle_dev_download(c, lab.ptr<unsigned char>(), d_out.p, n * 3), c);
    return lab;
}

Image lab2bgr8_device(const Image& lab) {
    if (lab.channels() != 3 || lab.depth() != NLE_8U) throw std::runtime_error("lab2bgr8: 8UC3 image expected");
    nle_ctx* c = shared_ctx();
    const size_t n = lab.total();
    Dev d_in(c, n * 3), d_out(c, n * 3);
    check(nle_dev_upload(c, d_in.p, lab.ptr<unsigned char>(), n * 3), c);
    check(nle_lab2bgr8(c, d_in.u8(), nullptr, (long long)n, d_out.u8()), c);
    Image bgr(lab.rows, lab.cols, NLE_8U, 3);
    check(nle_dev_download(c, bgr.ptr<unsigned char>(), d_out.p, n * 3), c);
    return bgr;
}

// ---- the bilateral prefilter of the denoise wrapper (src/filter.cpp:371, 535) ----
namespace {
int reflect101(int i, int n) {  // cv::BORDER_DEFAULT
    if (n == 1) return 0;
    const int period = 2 * n - 2;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}
}  // namespace

Image bilateralFilter8(const Image& plane, double sigmaColor, double sigmaSpace) {
    if (plane.channels() != 1 || plane.depth() != NLE_8U) throw std::runtime_error("bilateralFilter8: 8UC1 image expected");
    int radius = 0;
    nle_bilateral_tables(sigmaColor, sigmaSpace, &radius, nullptr, nullptr);
    const int d = 2 * radius + 1, H = plane.rows, W = plane.cols;
    std::vector<float> sw((size_t)d * d), cw(256);
    nle_bilateral_tables(sigmaColor, sigmaSpace, &radius, sw.data(), cw.data());
    Image out(H, W, NLE_8U, 1);
    std::vector<int> ry(d), rx(d);
    for (int y = 0; y < H; ++y) {
        for (int i = 0; i < d; ++i) ry[i] = reflect101(y - radius + i, H);
        for (int x = 0; x < W; ++x) {
            for (int j = 0; j < d; ++j) rx[j] = reflect101(x - radius + j, W);
            const float v0 = (float)plane.at<unsigned char>(y, x);
            volatile float sum = 0.f, wsum = 0.f;  // volatile: one rounding per operation, like the device kernel
            for (int i = 0; i < d; ++i)
                for (int j = 0; j < d; ++j) {
                    const float s = sw[(size_t)i * d + j];
                    if (s == 0.f) continue;
                    const float v = (float)plane.at<unsigned char>(ry[i], rx[j]);
                    volatile float w = s * cw[(int)std::fabs(v - v0)];
                    volatile float vw = v * w;
                    sum = sum + vw;
                    wsum = wsum + w;
                }
            volatile float q = sum / wsum;
            out.at<unsigned char>(y, x) = (unsigned char)std::nearbyint((float)q);
        }
    }
    return out;
}

Image bilateralFilter8_device(const Image& plane, double sigmaColor, double sigmaSpace) {
    if (plane.channels() != 1 || plane.depth() != NLE_8U) throw std::runtime_error("bilateralFilter8: 8UC1 image expected");
    nle_ctx* c = shared_ctx();
    const size_t n = plane.total();
    std::vector<float> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = (float)plane.ptr<unsigned char>()[i];
    Dev d_in(c, n * 4), d_out(c, n * 4);
    check(nle_dev_upload(c, d_in.p, h.data(), n * 4), c);
    check(nle_bilateral8(c, d_in.f(), plane.rows, plane.cols, sigmaColor, sigmaSpace, d_out.f()), c);
    check(nle_dev_download(c, h.data(), d_out.p, n * 4), c);
    Image out(plane.rows, plane.cols, NLE_8U, 1);
    for (size_t i = 0; i < n; ++i) out.ptr<unsigned char>()[i] = (unsigned char)h[i];
    return out;
}

}  // namespace nle
