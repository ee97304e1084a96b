// `enhance` CLI -- same argv, stdout and exit codes as the reference's src/enhance.cpp:12-52:
//   enhance <image> <output> <# row samples> <# col samples> <hx> <hy> <# sinkhorn iterations>
//           <# eigen vectors> <weight 1> [<weight 2> ...]
// Differences: runs headless (no imshow / waitKey, src/enhance.cpp:48-49), reads BMP/PPM and writes
// BMP/PPM/PNG through nle/image_io.hpp instead of OpenCV.  The hot path runs on the GPU through
// libnle_hip.so.  New here: leading options; nlecli::kOptions (cli_common.hpp) lists them.  With `--region` the positional
// weights are the background's; `--nystrom-report` prints one more stdout line with the Nystrom residual of the sample grid
// (mean, max and its pixel, share of pixels above 0.5) and `--nystrom-map FILE` writes the map as an 8-bit grey image,
// round(255 clamp(r, 0, 1)); `--deep` and `--tonemap` print the same banners.  `--shadows`, `--highlights`, `--auto-levels`
// and `--equalise` pass the base layer through a tone curve (nle::ToneOptions); with either of the last two one more stdout
// line follows the banner, `Tone curve: levels <lo> <hi>`: the range the curve was laid over.  `--segments C` lets the trained
// filter propose C regions (NLEFilter::segment): after the banner `Segments: <C> iterations <I> converged <yes|no> objective
// <J>` and one line `Segment <c>: <n> pixels, mean L <m>` per segment; `--segment-map FILE` writes the labels as an 8-bit grey
// image, segment c at round(255 c / (C - 1)); `--segment-weights c:w1,w2,...` gives segment c layer weights of its own
// (NLEFilter::enhanceSegments) -- without one the image written is the plain command's, byte for byte.  Two runs give the same
// labels: the first to look at the map and the lines, the second with weights.  `--local TARGET:key=value,...` gives a
// region -- a mask, or segment @c of `--segments C` -- the whole edit of its own (NLEFilter::enhanceLocal /
// enhanceSegmentsLocal): weights, residual, gain, sigma, shadows, highlights, saturation; what a spec does not name is the
// background's, which is the positional weights, the detail options, `--shadows`, `--highlights` and `--saturation`.
// `--local-auto ROW:levels=P[,equalise=A]` lays row ROW's base curve (0 the background, m the m-th `--local`) over the row's own
// membership-weighted histogram (nle::LocalEdit::clipPercent, equalise); each such row adds one stdout line, in ascending
// ROW: `Tone curve: row <ROW> levels <lo> <hi>`.
#include <algorithm>

#include "cli_common.hpp"

int main(int argc, char* argv[]) {
    nlecli::FilterArgs a;
    if (!nlecli::parse(argc, argv, 10, &a, nlecli::Tool::Enhance)) return 0;  // usage: src/enhance.cpp:15-18 (exit code 0 on purpose)
    const nle::Image image = nlecli::load(a);
    if (image.empty()) return 0;                        // src/enhance.cpp:34-37
    // the strokes: the first channel of every mask, read before anything touches the GPU
    std::vector<nle::Image> strokes;
    std::vector<std::vector<double>> regionWeights;
    // false, after one line on stderr, for a mask that cannot be read, has another size or marks no pixel
    const auto read_stroke = [&](const char* option, const std::string& path) {
        const nle::Image mask = nle::imread(path);
        if (mask.empty() || mask.rows != image.rows || mask.cols != image.cols) {
            std::cerr << argv[0] << ": " << option << " mask " << path
                      << (mask.empty() ? " cannot be read" : " does not have the image's size") << std::endl;
            return false;
        }
        nle::Image s(mask.rows, mask.cols, nle::NLE_8U, 1);
        const int ch = mask.channels();
        bool any = false;
        for (size_t i = 0; i < mask.total(); ++i) {
            s.ptr<unsigned char>()[i] = mask.ptr<unsigned char>()[i * ch];
            any = any || s.ptr<unsigned char>()[i] >= 128;
        }
        if (!any) {
            std::cerr << argv[0] << ": " << option << " mask " << path << " marks no pixel (no byte >= 128 in its first channel)"
                      << std::endl;
            return false;
        }
        strokes.push_back(s);
        return true;
    };
    for (const auto& r : a.regions) {
        if (!read_stroke("--region", r.mask)) return 2;
        regionWeights.push_back(r.weights);
    }
    // the rows of a local adjustment: one per mask in the order given, or one per segment that has a spec
    std::vector<nle::LocalEdit> localEdits;
    const bool localSegments = !a.locals.empty() && a.locals[0].segment >= 0;
    // (a segment without a spec takes the background's keys, not its --local-auto: ROW 0 is the background's row alone)
    if (localSegments) localEdits.assign((size_t)a.segments, nlecli::local_edit(a, nullptr));
    for (size_t k = 0; k < a.locals.size(); ++k) {
        const auto& l = a.locals[k];
        if (localSegments) {
            localEdits[(size_t)l.segment] = nlecli::local_edit_row(a, (int)k + 1);
        } else {
            if (!read_stroke("--local", l.target)) return 2;
            localEdits.push_back(nlecli::local_edit_row(a, (int)k + 1));
        }
    }
    nle::NLEFilter filter;
    filter.patchRadius = a.patchRadius;
    filter.sampler = a.sampler;
    filter.exact = a.exact;
    filter.chromaBandwidth = a.chroma;
    filter.keepTrainPlane = a.segments != 0;  // segment() starts from the plane the train ran on
    if (a.tonemap) filter.trainForToneMapping(image, a.rowSamples, a.colSamples, a.hx, a.hy, a.sinkhornIters, a.eigenVectors);
    else filter.trainForEnhancement(image, a.rowSamples, a.colSamples, a.hx, a.hy, a.sinkhornIters, a.eigenVectors);
    nle::Image labels;
    std::vector<std::vector<double>> segmentWeights((size_t)a.segments);
    if (a.segments) {
        nle::SegmentOptions o;
        o.count = a.segments, o.spread = a.segmentSpread, o.maxIterations = a.segmentIterations;
        labels = filter.segment(o);
        for (size_t k = 0; k < a.segmentOf.size(); ++k) segmentWeights[a.segmentOf[k]] = a.segmentWeights[k].weights;
    }
    // (inactive detail and tone options are the plain methods; segments without weights of their own leave the plain edit)
    const nle::Image result = a.tonemap                  ? filter.toneMap(image, a.extra, a.tonemapSaturation, a.detail)
                              : localSegments             ? filter.enhanceSegmentsLocal(image, nlecli::local_edit_row(a, 0), localEdits)
                              : !a.locals.empty()         ? filter.enhanceLocal(image, strokes, localEdits, nlecli::local_edit_row(a, 0),
                                                                                a.regionSpread, a.regionFloor)
                              : !a.segmentWeights.empty() ? filter.enhanceSegments(image, a.extra, segmentWeights)
                              : strokes.empty()           ? filter.enhance(image, a.extra, a.detail, a.tone)  // the weights are argv[9..]
                                                          : filter.enhanceRegions(image, strokes, regionWeights, a.extra, a.regionSpread,
                                                                                  a.regionFloor);
    nlecli::report(filter);
    const int rc = nlecli::finish(a, result, "Done. Press any key in result window to exit.");  // src/enhance.cpp:45
    if (a.segments) {
        const nle::SegmentReport s = filter.lastSegments();
        std::cout << "Segments: " << a.segments << " iterations " << s.iterations << " converged " << (s.converged ? "yes" : "no")
                  << " objective " << s.objective << std::endl;
        for (int c = 0; c < a.segments; ++c)
            std::cout << "Segment " << c << ": " << s.counts[c] << " pixels, mean L " << s.meanL[c] << std::endl;
        if (!a.segmentMap.empty()) {
            nle::Image grey(image.rows, image.cols, nle::NLE_8U, 3);  // grey as three equal channels (what the writers take)
            for (size_t i = 0; i < image.total(); ++i) {
                const unsigned char v = (unsigned char)std::nearbyint(255.0 * labels.ptr<unsigned char>()[i] / (a.segments - 1));
                grey.ptr<unsigned char>()[3 * i] = grey.ptr<unsigned char>()[3 * i + 1] = grey.ptr<unsigned char>()[3 * i + 2] = v;
            }
            if (!nle::imwrite(a.segmentMap, grey)) {
                std::cerr << "Failed to write " << a.segmentMap << std::endl;
                return 1;
            }
        }
    }
    if (a.toneLine) {
        const nle::ToneLevels t = filter.lastToneCurve();
        std::cout << "Tone curve: levels " << t.lo << " " << t.hi << std::endl;
    }
    if (!a.localAutos.empty()) {  // one line per row that has --local-auto, in ascending ROW
        const std::vector<nle::ToneLevels> levels = filter.lastLocalLevels();
        for (int row = 0; row <= (int)a.locals.size(); ++row)
            for (const auto& u : a.localAutos)
                if (u.row == row) {
                    const nle::ToneLevels t = levels.at((size_t)nlecli::local_auto_row(a, u));
                    std::cout << "Tone curve: row " << row << " levels " << t.lo << " " << t.hi << std::endl;
                }
    }
    if (a.nystromReport) {  // after the reference's banners: one line, and the map as an 8-bit grey image
        const nle::NLEFilter::Residual res = filter.nystromResidual(image, a.rowSamples, a.colSamples, a.hx, a.hy);
        const double n = (double)image.total();
        std::cout << "Nystrom residual: mean " << res.sum / n << " max " << res.max << " at (" << res.argmax / image.cols << ", "
                  << res.argmax % image.cols << ") share above 0.5: " << (double)res.count / n << std::endl;
        if (!a.nystromMap.empty()) {
            nle::Image grey(image.rows, image.cols, nle::NLE_8U, 3);  // grey as three equal channels (what the writers take)
            for (size_t i = 0; i < image.total(); ++i) {
                const double r = std::min(1.0, std::max(0.0, res.map.ptr<double>()[i]));
                const unsigned char v = (unsigned char)std::floor(255.0 * r + 0.5);
                grey.ptr<unsigned char>()[3 * i] = grey.ptr<unsigned char>()[3 * i + 1] = grey.ptr<unsigned char>()[3 * i + 2] = v;
            }
            if (!nle::imwrite(a.nystromMap, grey)) {
                std::cerr << "Failed to write " << a.nystromMap << std::endl;
                return 1;
            }
        }
    }
    return rc;
}
