// Shared shell of the two command-line tools (enhance, denoise): both take
//   <image> <output> <# row samples> <# col samples> <hx> <hy> <# sinkhorn iterations> <# eigen vectors> ...
// print the same usage line when too few arguments are given, parse numbers with std::stoi / std::stod (garbage
// throws, like the reference: src/enhance.cpp:20-31, src/denoise.cpp:19-31) and return 0 on the two soft failures
// (usage, unreadable image) for drop-in compatibility.  New here: optional LEADING `--patch-radius R` (patch affinities,
// NLEFilter::patchRadius), `--sampler grid|farthest|residual` (NLEFilter::sampler) and the flag `--exact` (NLEFilter::exact, no
// value; not with a non-zero radius or a sampler other than the grid) and, for enhance only, `--chroma HC` (chroma-aware affinities,
// NLEFilter::chromaBandwidth: a finite number > 0; not with --exact or a radius above NLE_CHROMA_PATCH_RADIUS_MAX), in any order; reference command lines never start with
// `--`, so they parse exactly as before.  An invalid value prints a message to stderr and exits with status 2 before
// anything touches the GPU.  For enhance only, region edits (NLEFilter::enhanceRegions): `--region MASK:w1,w2,...`, up to
// NLE_REGION_MAX times (split at the last `:`; MASK any image the readers decode, its first channel is the stroke; as many
// weights as positional ones, which are the background's), `--region-spread T` and `--region-floor F` (finite, > 0; only
// with a region); the flag `--nystrom-report` with its optional `--nystrom-map FILE` (NLEFilter::nystromResidual; not
// with --exact); and the flag `--deep` (no value): the input is read with imread16 -- a 16-bit PNG keeps every sample -- and
// the result is written as a 16-bit PNG (the output name must end in .png; not with --region); and the flag `--tonemap`
// (no value) with its optional `--tonemap-saturation S` (a finite number in (0, 2]): the input is an HDR file read with
// imreadHDR, the positional weights are the layer weights of NLEFilter::toneMap -- the last one is the base compression --
// and the result is a 16-bit PNG (not with --chroma, --region, --deep or --nystrom-report); and `--residual-weight WR` (a
// finite number), `--detail-gain A` (finite, in [0, NLE_DETAIL_GAIN_MAX]) and `--detail-sigma S` (finite, >= 0):
// nle::DetailOptions of NLEFilter::enhance / toneMap, with --deep and --tonemap too (a gain other than 1 needs a sigma > 0;
// not with --region).  For denoise only, the MSE-guided denoiser (nle::DenoiseOptions): `--prefilter bilateral|nlm`, the flag
// `--glide` (no value), `--noise-sigma S` (finite, >= 0; needs --glide or --prefilter nlm) and `--nlm-h H` (finite, > 0; needs
// --prefilter nlm); under --glide the positional shrink factor is the upper end of the searched range.
#pragma once

#include <cctype>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "nle.h"
#include "nle/filter.hpp"
#include "nle/image_io.hpp"

namespace nlecli {

struct FilterArgs {
    std::string input, output;
    int rowSamples = 0, colSamples = 0, sinkhornIters = 0, eigenVectors = 0;
    double hx = 0, hy = 0;
    std::vector<double> extra;  // everything after the eighth argument, as doubles
    int patchRadius = 0;        // --patch-radius R
    int sampler = NLE_SAMPLER_GRID;  // --sampler grid|farthest|residual
    bool exact = false;              // --exact
    double chroma = 0;               // --chroma HC (enhance only)
    // --region MASK:w1,w2,... (enhance only, repeatable), --region-spread T, --region-floor F
    struct Region {
        std::string mask;
        std::vector<double> weights;
    };
    std::vector<Region> regions;
    double regionSpread = 4, regionFloor = 0.05;
    bool deep = false;               // --deep (enhance only): 16-bit PNG in, 16-bit PNG out
    bool tonemap = false;            // --tonemap (enhance only): Radiance / PFM in, 16-bit PNG out
    double tonemapSaturation = 1;    // --tonemap-saturation S (with --tonemap)
    nle::DetailOptions detail;       // --residual-weight WR, --detail-gain A, --detail-sigma S (enhance only)
    nle::DenoiseOptions denoise;     // --prefilter bilateral|nlm, --glide, --noise-sigma S, --nlm-h H (denoise only)
    bool nystromReport = false;  // --nystrom-report (enhance only)
    std::string nystromMap;      // --nystrom-map FILE (with --nystrom-report)
};

// a finite number > 0, or exit 2
inline double positive_option(const char* prog, const std::string& opt, const std::string& v) {
    char* end = nullptr;
    const double x = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
    if (v.empty() || *end != '\0' || !std::isfinite(x) || !(x > 0)) {
        std::cerr << prog << ": " << opt << " takes a finite number > 0, got '" << v << "'" << std::endl;
        std::exit(2);
    }
    return x;
}

// false (after printing the usage line to stderr) when fewer than `min_argc` arguments were given
// allow_chroma: the tool takes `--chroma HC` (enhance); otherwise the option is refused (denoise estimates a and b)
// allow_regions: the tool takes the region options (enhance); otherwise they are refused (denoise has no layer weights)
// allow_nystrom: the tool takes `--nystrom-report` / `--nystrom-map FILE` (enhance); otherwise they are refused
// allow_deep: the tool takes `--deep` (enhance); otherwise it is refused (denoise has no 16-bit path)
// allow_tonemap: the tool takes `--tonemap` / `--tonemap-saturation S` (enhance); otherwise they are refused
// allow_detail: the tool takes `--residual-weight WR` / `--detail-gain A` / `--detail-sigma S` (enhance); otherwise refused
// allow_denoise: the tool takes `--prefilter` / `--glide` / `--noise-sigma` / `--nlm-h` (denoise); otherwise they are refused
inline bool parse(int argc, char* argv[], int min_argc, FilterArgs* a, bool allow_chroma = false,
                  bool allow_regions = false, bool allow_nystrom = false, bool allow_deep = false,
                  bool allow_tonemap = false, bool allow_detail = false, bool allow_denoise = false) {
    std::vector<char*> shifted;
    int first = 1;  // the first argument after the leading options
    bool spreadGiven = false, floorGiven = false, saturationGiven = false;
    std::string detailGiven;  // the last of --residual-weight / --detail-gain / --detail-sigma seen
    bool noiseSigmaGiven = false, nlmHGiven = false;
    while (first < argc) {
        const std::string opt = argv[first];
        if (opt == "--exact") {
            a->exact = true;
            first += 1;
            continue;
        }
        if (opt.rfind("--exact=", 0) == 0) {
            std::cerr << argv[0] << ": --exact takes no value, got '" << opt << "'" << std::endl;
            std::exit(2);
        }
        if (opt == "--deep" || opt.rfind("--deep=", 0) == 0) {
            if (!allow_deep) {
                std::cerr << argv[0] << ": --deep is not supported here: deep colour (16 bit) is built for enhance only" << std::endl;
                std::exit(2);
            }
            if (opt != "--deep") {
                std::cerr << argv[0] << ": --deep takes no value, got '" << opt << "'" << std::endl;
                std::exit(2);
            }
            a->deep = true;
            first += 1;
            continue;
        }
        if (opt.rfind("--tonemap", 0) == 0) {
            if (!allow_tonemap) {
                std::cerr << argv[0] << ": " << opt << " is not supported here: --tonemap (HDR tone mapping) is built for enhance only"
                          << std::endl;
                std::exit(2);
            }
            if (opt == "--tonemap") {
                a->tonemap = true;
                first += 1;
                continue;
            }
            if (opt != "--tonemap-saturation") {
                std::cerr << argv[0] << ": --tonemap takes no value and --tonemap-saturation takes a number, got '" << opt << "'"
                          << std::endl;
                std::exit(2);
            }
            const std::string v = first + 1 < argc ? argv[first + 1] : "";
            char* end = nullptr;
            const double x = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
            if (v.empty() || *end != '\0' || !std::isfinite(x) || !(x > 0) || x > 2) {
                std::cerr << argv[0] << ": --tonemap-saturation takes a finite number in (0, 2], got '" << v << "'" << std::endl;
                std::exit(2);
            }
            a->tonemapSaturation = x;
            saturationGiven = true;
            first += 2;
            continue;
        }
        if (opt == "--nystrom-report" || opt == "--nystrom-map" || opt.rfind("--nystrom-report=", 0) == 0) {
            if (!allow_nystrom) {
                std::cerr << argv[0] << ": " << opt << " is not supported here: the residual report belongs to enhance" << std::endl;
                std::exit(2);
            }
            if (opt == "--nystrom-report") {
                a->nystromReport = true;
                first += 1;
                continue;
            }
            const std::string file = first + 1 < argc ? argv[first + 1] : "";
            if (opt != "--nystrom-map" || file.empty() || file.rfind("--", 0) == 0) {
                std::cerr << argv[0] << ": --nystrom-report takes no value and --nystrom-map takes a file name, got '" << opt
                          << (opt == "--nystrom-map" ? " " + file : "") << "'" << std::endl;
                std::exit(2);
            }
            a->nystromMap = file;
            first += 2;
            continue;
        }
        if (opt == "--residual-weight" || opt == "--detail-gain" || opt == "--detail-sigma") {
            if (!allow_detail) {
                std::cerr << argv[0] << ": " << opt << " is not supported here: the detail options weigh layers, which this tool "
                          << "does not take" << std::endl;
                std::exit(2);
            }
            const std::string v = first + 1 < argc ? argv[first + 1] : "";
            char* end = nullptr;
            const double x = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
            const bool number = !v.empty() && *end == '\0' && std::isfinite(x);
            if (opt == "--residual-weight") {
                if (!number) {
                    std::cerr << argv[0] << ": --residual-weight takes a finite number, got '" << v << "'" << std::endl;
                    std::exit(2);
                }
                a->detail.residualWeight = x;
            } else if (opt == "--detail-gain") {
                if (!number || x < 0 || x > NLE_DETAIL_GAIN_MAX) {
                    std::cerr << argv[0] << ": --detail-gain takes a finite number in [0, " << NLE_DETAIL_GAIN_MAX << "], got '" << v
                              << "'" << std::endl;
                    std::exit(2);
                }
                a->detail.gain = x;
            } else {
                if (!number || x < 0) {
                    std::cerr << argv[0] << ": --detail-sigma takes a finite number >= 0, got '" << v << "'" << std::endl;
                    std::exit(2);
                }
                a->detail.sigma = x;
            }
            detailGiven = opt;
            first += 2;
            continue;
        }
        if (opt == "--glide" || opt.rfind("--glide=", 0) == 0 || opt == "--prefilter" || opt == "--noise-sigma" || opt == "--nlm-h") {
            if (!allow_denoise) {
                std::cerr << argv[0] << ": " << opt << " is not supported here: the pre-filter and the MSE-guided shrinkage belong "
                          << "to denoise" << std::endl;
                std::exit(2);
            }
            if (opt.rfind("--glide", 0) == 0) {
                if (opt != "--glide") {
                    std::cerr << argv[0] << ": --glide takes no value, got '" << opt << "'" << std::endl;
                    std::exit(2);
                }
                a->denoise.glide = true;
                first += 1;
                continue;
            }
            const std::string v = first + 1 < argc ? argv[first + 1] : "";
            if (opt == "--prefilter") {
                if (v != "bilateral" && v != "nlm") {
                    std::cerr << argv[0] << ": --prefilter takes 'bilateral' or 'nlm', got '" << v << "'" << std::endl;
                    std::exit(2);
                }
                a->denoise.prefilter = v == "nlm" ? NLE_PREFILTER_NLM : NLE_PREFILTER_BILATERAL;
            } else if (opt == "--noise-sigma") {
                char* end = nullptr;
                const double x = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
                if (v.empty() || *end != '\0' || !std::isfinite(x) || x < 0) {
                    std::cerr << argv[0] << ": --noise-sigma takes a finite number >= 0, got '" << v << "'" << std::endl;
                    std::exit(2);
                }
                a->denoise.noiseSigma = x;
                noiseSigmaGiven = true;
            } else {
                a->denoise.nlmH = positive_option(argv[0], opt, v);
                nlmHGiven = true;
            }
            first += 2;
            continue;
        }
        const bool regionOpt = opt == "--region" || opt == "--region-spread" || opt == "--region-floor";
        if (opt != "--patch-radius" && opt != "--sampler" && opt != "--chroma" && !regionOpt) break;
        const std::string v = first + 1 < argc ? argv[first + 1] : "";
        if (regionOpt) {
            if (!allow_regions) {
                std::cerr << argv[0] << ": " << opt << " is not supported here: region edits give layer weights, which this "
                          << "tool does not take" << std::endl;
                std::exit(2);
            }
            if (opt == "--region-spread") {
                a->regionSpread = positive_option(argv[0], opt, v);
                spreadGiven = true;
            } else if (opt == "--region-floor") {
                a->regionFloor = positive_option(argv[0], opt, v);
                floorGiven = true;
            } else {
                const size_t colon = v.rfind(':');
                FilterArgs::Region r;
                bool ok = colon != std::string::npos && colon > 0 && colon + 1 < v.size();
                if (ok) {
                    r.mask = v.substr(0, colon);
                    const std::string list = v.substr(colon + 1) + ",";
                    for (size_t p = 0, q; ok && (q = list.find(',', p)) != std::string::npos; p = q + 1) {
                        const std::string w = list.substr(p, q - p);
                        char* end = nullptr;
                        const double x = w.empty() ? 0.0 : std::strtod(w.c_str(), &end);
                        ok = !w.empty() && *end == '\0' && std::isfinite(x);
                        r.weights.push_back(x);
                    }
                }
                if (!ok) {
                    std::cerr << argv[0] << ": --region takes MASK:w1,w2,... (an image and finite weights), got '" << v << "'"
                              << std::endl;
                    std::exit(2);
                }
                if ((int)a->regions.size() == NLE_REGION_MAX) {
                    std::cerr << argv[0] << ": --region can be given at most " << NLE_REGION_MAX << " times" << std::endl;
                    std::exit(2);
                }
                a->regions.push_back(r);
            }
            first += 2;
            continue;
        }
        if (opt == "--chroma") {
            if (!allow_chroma) {
                std::cerr << argv[0] << ": --chroma is not supported here: the a and b planes are what this tool estimates"
                          << std::endl;
                std::exit(2);
            }
            char* end = nullptr;
            const double hc = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
            if (v.empty() || *end != '\0' || !std::isfinite(hc) || !(hc > 0)) {
                std::cerr << argv[0] << ": --chroma takes a finite number > 0 (the chroma bandwidth), got '" << v << "'"
                          << std::endl;
                std::exit(2);
            }
            a->chroma = hc;
        } else if (opt == "--patch-radius") {
            char* end = nullptr;
            const long r = v.empty() ? -1 : std::strtol(v.c_str(), &end, 10);
            if (v.empty() || *end != '\0' || r < 0 || r > NLE_PATCH_RADIUS_MAX) {
                std::cerr << argv[0] << ": --patch-radius takes an integer in [0, " << NLE_PATCH_RADIUS_MAX << "], got '" << v
                          << "'" << std::endl;
                std::exit(2);
            }
            a->patchRadius = (int)r;
        } else {
            if (v != "grid" && v != "farthest" && v != "residual") {
                std::cerr << argv[0] << ": --sampler takes 'grid', 'farthest' or 'residual', got '" << v << "'" << std::endl;
                std::exit(2);
            }
            a->sampler = v == "grid" ? NLE_SAMPLER_GRID : v == "farthest" ? NLE_SAMPLER_FARTHEST : NLE_SAMPLER_RESIDUAL;
        }
        first += 2;
    }
    if (noiseSigmaGiven && !a->denoise.glide && a->denoise.prefilter != NLE_PREFILTER_NLM) {
        std::cerr << argv[0] << ": --noise-sigma needs --glide or --prefilter nlm (nothing else uses a noise level)" << std::endl;
        std::exit(2);
    }
    if (nlmHGiven && a->denoise.prefilter != NLE_PREFILTER_NLM) {
        std::cerr << argv[0] << ": --nlm-h needs --prefilter nlm" << std::endl;
        std::exit(2);
    }
    if (a->exact && (a->patchRadius != 0 || a->sampler != NLE_SAMPLER_GRID)) {
        std::cerr << argv[0] << ": --exact uses no samples and single-pixel affinities: it does not combine with "
                  << "--patch-radius R > 0, --sampler farthest or --sampler residual" << std::endl;
        std::exit(2);
    }
    if (a->chroma != 0 && (a->exact || a->patchRadius > NLE_CHROMA_PATCH_RADIUS_MAX)) {
        std::cerr << argv[0] << ": --chroma does not combine with --exact or with --patch-radius R > "
                  << NLE_CHROMA_PATCH_RADIUS_MAX << std::endl;
        std::exit(2);
    }
    if (!a->nystromMap.empty() && !a->nystromReport) {
        std::cerr << argv[0] << ": --nystrom-map needs --nystrom-report" << std::endl;
        std::exit(2);
    }
    if (a->nystromReport && a->exact) {
        std::cerr << argv[0] << ": --nystrom-report and --nystrom-map do not combine with --exact: the exact filter has no "
                  << "Nystrom extension" << std::endl;
        std::exit(2);
    }
    if (a->deep && !a->regions.empty()) {
        std::cerr << argv[0] << ": --deep does not combine with --region: region edits take an 8-bit image" << std::endl;
        std::exit(2);
    }
    if (saturationGiven && !a->tonemap) {
        std::cerr << argv[0] << ": --tonemap-saturation needs --tonemap" << std::endl;
        std::exit(2);
    }
    if (a->tonemap && (a->chroma != 0 || !a->regions.empty() || a->deep || a->nystromReport)) {
        std::cerr << argv[0] << ": --tonemap does not combine with --chroma, --region, --deep or --nystrom-report: those take "
                  << "an 8-bit or 16-bit sRGB image" << std::endl;
        std::exit(2);
    }
    if (a->detail.gain != 1 && !(a->detail.sigma > 0)) {
        std::cerr << argv[0] << ": --detail-gain other than 1 needs --detail-sigma S > 0 (the amplitude the gain acts below)"
                  << std::endl;
        std::exit(2);
    }
    if (!detailGiven.empty() && !a->regions.empty()) {
        std::cerr << argv[0] << ": " << detailGiven << " does not combine with --region: region edits have no residual layer "
                  << "and no detail curve" << std::endl;
        std::exit(2);
    }
    if ((spreadGiven || floorGiven) && a->regions.empty()) {
        std::cerr << argv[0] << ": --region-spread and --region-floor need at least one --region" << std::endl;
        std::exit(2);
    }
    if (first > 1) {
        shifted.push_back(argv[0]);  // the rest parses as a reference command line
        for (int i = first; i < argc; ++i) shifted.push_back(argv[i]);
        shifted.push_back(nullptr);
        argc -= first - 1;
        argv = shifted.data();
    }
    if (argc < min_argc) {
        std::cerr << "Usage: " << argv[0]
                  << " <image> <output> <# row samples> <# col samples> <hx> <hy> <# sinkhorn iterations> <# eigen "
                     "vectors> <weight 1> <weight 2> <weight 3> <weight 4>"
                  << std::endl;
        return false;
    }
    a->input = argv[1];
    a->output = argv[2];
    if (a->deep || a->tonemap) {  // the only 16-bit writer is the PNG one
        const std::string& o = a->output;
        std::string ext = o.size() >= 4 ? o.substr(o.size() - 4) : "";
        for (char& ch : ext) ch = (char)std::tolower((unsigned char)ch);
        if (ext != ".png") {
            std::cerr << argv[0] << ": " << (a->deep ? "--deep" : "--tonemap")
                      << " writes a 16-bit PNG: the output name must end in .png, got '" << o << "'" << std::endl;
            std::exit(2);
        }
    }
    int* ints[] = {&a->rowSamples, &a->colSamples, nullptr, nullptr, &a->sinkhornIters, &a->eigenVectors};
    double* reals[] = {nullptr, nullptr, &a->hx, &a->hy, nullptr, nullptr};
    for (int i = 0; i < 6; ++i) {
        if (ints[i]) *ints[i] = std::stoi(argv[3 + i]);
        else *reals[i] = std::stod(argv[3 + i]);
    }
    for (int i = 9; i < argc; ++i) a->extra.push_back(std::stod(argv[i]));
    if (a->detail.active() && (int)a->extra.size() > NLE_REGION_LAYERS_MAX) {
        std::cerr << argv[0] << ": " << detailGiven << " takes at most " << NLE_REGION_LAYERS_MAX << " weights, got "
                  << a->extra.size() << std::endl;
        std::exit(2);
    }
    if (!a->regions.empty()) {  // every region has the background's weight count
        if ((int)a->extra.size() > NLE_REGION_LAYERS_MAX) {
            std::cerr << argv[0] << ": --region takes at most " << NLE_REGION_LAYERS_MAX << " weights, got "
                      << a->extra.size() << std::endl;
            std::exit(2);
        }
        for (const auto& r : a->regions)
            if (r.weights.size() != a->extra.size()) {
                std::cerr << argv[0] << ": --region " << r.mask << " has " << r.weights.size() << " weights, the command line "
                          << "has " << a->extra.size() << std::endl;
                std::exit(2);
            }
    }
    return true;
}

// reads the input (empty image + message on stderr if that fails)
inline nle::Image load(const FilterArgs& a) {
    nle::Image image = a.tonemap ? nle::imreadHDR(a.input) : a.deep ? nle::imread16(a.input) : nle::imread(a.input);
    if (image.empty()) std::cerr << "Failed to read file from " << a.input << std::endl;
    return image;
}

// NLE_REPORT=<path> (an environment variable, so that reference-style command lines stay valid): one JSON object
// with what the train decided (nle_filter_diag), the kept eigenvalues and the per-stage milliseconds
inline void report(const nle::NLEFilter& filter) {
    const char* path = std::getenv("NLE_REPORT");
    if (!path || !*path) return;
    int d[8];
    double ms[6] = {0, 0, 0, 0, 0, 0};
    filter.diag(d);
    filter.timings(ms);
    const nle::Vec ev = filter.eigvals();
    std::ofstream os(path);
    os.precision(17);
    os << "{\"formulation\": " << d[0] << ", \"p\": " << d[1] << ", \"r_Ka\": " << d[2] << ", \"r_Wa\": " << d[3]
       << ", \"r_Q\": " << d[4] << ", \"K\": " << d[5] << ", \"chol_Ka\": " << d[6] << ", \"chol_Wa\": " << d[7]
       << ", \"eigvals\": [";
    for (int i = 0; i < ev.size(); ++i) os << (i ? ", " : "") << ev(i);
    os << "], \"ms\": {\"samples\": " << ms[0] << ", \"sinkhorn\": " << ms[1] << ", \"gram\": " << ms[2]
       << ", \"project\": " << ms[3] << ", \"host\": " << ms[4] << ", \"train_total\": " << ms[5] << "}";
    const nle::DenoiseReport g = filter.lastDenoiseReport();  // denoise --glide: (sigma, k, MSE(k)) of L, a and b
    if (g.valid) {
        os << ", \"glide\": {";
        const char* names[3] = {"L", "a", "b"};
        for (int ch = 0; ch < 3; ++ch)
            os << (ch ? ", " : "") << "\"" << names[ch] << "\": {\"sigma\": " << g.sigma[ch] << ", \"k\": " << g.k[ch]
               << ", \"mse\": " << g.mse[ch] << "}";
        os << "}";
    }
    os << "}" << std::endl;
}

// `banner`: the line the reference prints before it writes the file (src/enhance.cpp:45, src/denoise.cpp:45); the
// window and the key press it announces do not exist here (headless)
inline int finish(const FilterArgs& a, const nle::Image& result, const char* banner) {
    std::cout << banner << std::endl;
    if (nle::imwrite(a.output, result)) return 0;
    std::cerr << "Failed to write " << a.output << std::endl;
    return 1;
}

}  // namespace nlecli
