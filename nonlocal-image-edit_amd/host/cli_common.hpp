// Shared shell of the two command-line tools (enhance, denoise): both take
//   <image> <output> <# row samples> <# col samples> <hx> <hy> <# sinkhorn iterations> <# eigen vectors> ...
// print the same usage line when too few arguments are given, parse numbers with std::stoi / std::stod (garbage
// throws, like the reference: src/enhance.cpp:20-31, src/denoise.cpp:19-31) and return 0 on the two soft failures
// (usage, unreadable image) for drop-in compatibility.  New here: LEADING options, in any order, one row of kOptions each
// (the table says what an option is, which tool takes it and what it takes); reference command lines never start with
// `--`, so they parse exactly as before.  The first word that is no option ends them and is <image>.  An invalid value or
// combination prints one line to stderr and exits with status 2 before anything touches the GPU.
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
    nle::ToneOptions tone;           // --shadows S, --highlights Hh, --auto-levels P, --equalise A (enhance only)
    bool toneLine = false;           // --auto-levels or --equalise was given: one more stdout line, the curve's range
    nle::DenoiseOptions denoise;     // --prefilter bilateral|nlm, --glide, --noise-sigma S, --nlm-h H (denoise only)
    // --segments C (enhance only), --segment-spread T, --segment-iterations I, --segment-map FILE, --segment-weights
    // c:w1,w2,... (repeatable; Region::mask holds c as given, segmentOf its number)
    int segments = 0;
    double segmentSpread = 4;
    int segmentIterations = 40;
    std::string segmentMap;
    std::vector<Region> segmentWeights;
    std::vector<int> segmentOf;
    // --local TARGET:key=value[,key=value...] (enhance only, repeatable): TARGET a mask file or @c; `given` and `value` by
    // key in the order of kLocalKeys (entry 0, weights, keeps its values in `weights`); --saturation C: the background's
    struct Local {
        std::string target;
        int segment = -1;  // c of @c; -1: a mask
        std::vector<double> weights;
        bool given[7] = {false, false, false, false, false, false, false};
        double value[7] = {0, 0, 0, 0, 0, 0, 0};
    };
    std::vector<Local> locals;
    double saturation = 1;
    // --local-auto ROW:levels=P[,equalise=A] (enhance only, once per row): ROW 0 the background, m the m-th --local
    struct LocalAuto {
        std::string text;
        int row = 0;
        bool hasLevels = false, hasEqualise = false;
        double levels = -1, equalise = 0;
    };
    std::vector<LocalAuto> localAutos;
    bool nystromReport = false;  // --nystrom-report (enhance only)
    std::string nystromMap;      // --nystrom-map FILE (with --nystrom-report)
};

enum class Tool { Enhance = 1, Denoise = 2 };
constexpr int kEnhance = (int)Tool::Enhance, kDenoise = (int)Tool::Denoise, kBoth = kEnhance | kDenoise;

// what an option takes.  A flag is the word alone, `--flag=...` is refused; FlagAnySuffix also claims every other word
// that starts with its name (and refuses it).  The numbers are finite doubles: any, > 0, >= 0, in [lo, hi], in (lo, hi];
// Integer is a whole number in [lo, hi]; Word is one of `words`; FileName is a word that does not start with `--`; Region
// is MASK:w1,w2,... split at the last `:`, finite weights; SegmentWeights is c:w1,w2,... likewise, c a whole number in [lo, hi].
// Local is TARGET:key=value[,key=value...] split at the last `:`, the keys those of kLocalKeys.  LocalAuto is
// ROW:levels=P[,equalise=A], ROW a whole number in [lo, hi], either key alone allowed.
enum class Takes { Flag, FlagAnySuffix, Finite, Positive, NonNegative, Closed, HalfOpen, Integer, Word, FileName, Region, SegmentWeights, Local,
                   LocalAuto };

struct Word {
    const char* word;
    int value;
};
struct Value {  // a parsed value: the number (or the word's constant), the text as given, the region
    double x = 0;
    std::string text;
    FilterArgs::Region region;
    FilterArgs::Local local;
    FilterArgs::LocalAuto localAuto;
};

struct Option {
    const char* name;
    const char* what;  // one line on what it does
    int tools;         // kEnhance, kDenoise or kBoth
    Takes takes;
    double lo, hi;      // Closed, HalfOpen, Integer
    const Word* words;  // Word: ends with {nullptr, 0}
    void (*set)(FilterArgs&, const Value&);  // where the value goes
    const char* takesText;      // "<this> takes ...": the refusal of a bad value ends ", got '<value>'"
    const char* elsewhereText;  // the other tool's refusal: "<word> is not supported here: <this>"
    bool elsewhereSaysName = false;  // ... with the option's name in place of the word as given (--deep=1 reads --deep)
};

#define NLECLI_STR2(x) #x
#define NLECLI_STR(x) NLECLI_STR2(x)

inline const Word kSamplers[] = {{"grid", NLE_SAMPLER_GRID}, {"farthest", NLE_SAMPLER_FARTHEST}, {"residual", NLE_SAMPLER_RESIDUAL},
                                 {nullptr, 0}};
inline const Word kPrefilters[] = {{"bilateral", NLE_PREFILTER_BILATERAL}, {"nlm", NLE_PREFILTER_NLM}, {nullptr, 0}};
inline const char kRegionElsewhere[] = "region edits give layer weights, which this tool does not take";
inline const char kNystromTakes[] = "--nystrom-report takes no value and --nystrom-map takes a file name";
inline const char kNystromElsewhere[] = "the residual report belongs to enhance";
inline const char kTonemapElsewhere[] = "--tonemap (HDR tone mapping) is built for enhance only";
inline const char kDetailElsewhere[] = "the detail options weigh layers, which this tool does not take";
inline const char kToneElsewhere[] = "the base tone curve remaps a layer, which this tool does not take";
inline const char kSegmentElsewhere[] = "automatic regions propose where layer weights go, which this tool does not take";
inline const char kLocalElsewhere[] = "local adjustments edit layers and colour per region, which this tool does not take";
inline const char kDenoiseElsewhere[] = "the pre-filter and the MSE-guided shrinkage belong to denoise";

// One row per option.  What holds between options (--noise-sigma needs ..., --exact does not combine with ...) is the
// ordered list in parse(), after the loop.
inline const Option kOptions[] = {
    {"--patch-radius", "patch affinities of radius R (NLEFilter::patchRadius)", kBoth, Takes::Integer, 0, NLE_PATCH_RADIUS_MAX, nullptr,
     [](FilterArgs& a, const Value& v) { a.patchRadius = (int)v.x; },
     "--patch-radius takes an integer in [0, " NLECLI_STR(NLE_PATCH_RADIUS_MAX) "]", ""},
    {"--sampler", "how the Nystrom samples are chosen (NLEFilter::sampler)", kBoth, Takes::Word, 0, 0, kSamplers,
     [](FilterArgs& a, const Value& v) { a.sampler = (int)v.x; }, "--sampler takes 'grid', 'farthest' or 'residual'", ""},
    {"--exact", "the exact, Nystrom-free filter (NLEFilter::exact)", kBoth, Takes::Flag, 0, 0, nullptr,
     [](FilterArgs& a, const Value&) { a.exact = true; }, "--exact takes no value", ""},
    {"--chroma", "chroma-aware affinities of bandwidth HC (NLEFilter::chromaBandwidth)", kEnhance, Takes::Positive, 0, 0, nullptr,
     [](FilterArgs& a, const Value& v) { a.chroma = v.x; }, "--chroma takes a finite number > 0 (the chroma bandwidth)",
     "the a and b planes are what this tool estimates"},
    {"--region", "a region edit (NLEFilter::enhanceRegions): MASK is any image the readers decode, its first channel the stroke; as "
                 "many weights as positional ones, which are then the background's; up to NLE_REGION_MAX times",
     kEnhance, Takes::Region, 0, 0, nullptr, [](FilterArgs& a, const Value& v) { a.regions.push_back(v.region); },
     "--region takes MASK:w1,w2,... (an image and finite weights)", kRegionElsewhere},
    {"--region-spread", "how far a stroke spreads (enhanceRegions' spread)", kEnhance, Takes::Positive, 0, 0, nullptr,
     [](FilterArgs& a, const Value& v) { a.regionSpread = v.x; }, "--region-spread takes a finite number > 0", kRegionElsewhere},
    {"--region-floor", "the membership floor of the background (enhanceRegions' floor)", kEnhance, Takes::Positive, 0, 0, nullptr,
     [](FilterArgs& a, const Value& v) { a.regionFloor = v.x; }, "--region-floor takes a finite number > 0", kRegionElsewhere},
    {"--nystrom-report", "one more stdout line: the Nystrom residual of the sample grid (NLEFilter::nystromResidual)", kEnhance,
     Takes::Flag, 0, 0, nullptr, [](FilterArgs& a, const Value&) { a.nystromReport = true; }, kNystromTakes, kNystromElsewhere},
    {"--nystrom-map", "the residual map as an 8-bit grey image, written to FILE", kEnhance, Takes::FileName, 0, 0, nullptr,
     [](FilterArgs& a, const Value& v) { a.nystromMap = v.text; }, kNystromTakes, kNystromElsewhere},
    {"--deep", "deep colour: the input is read with imread16, the result is a 16-bit PNG", kEnhance, Takes::Flag, 0, 0, nullptr,
     [](FilterArgs& a, const Value&) { a.deep = true; }, "--deep takes no value", "deep colour (16 bit) is built for enhance only", true},
    {"--tonemap", "HDR tone mapping (NLEFilter::toneMap): the input is read with imreadHDR, the weights are the layer weights -- "
                  "the last one is the base compression -- and the result is a 16-bit PNG",
     kEnhance, Takes::FlagAnySuffix, 0, 0, nullptr, [](FilterArgs& a, const Value&) { a.tonemap = true; },
     "--tonemap takes no value and --tonemap-saturation takes a number", kTonemapElsewhere},
    {"--tonemap-saturation", "toneMap's colour saturation", kEnhance, Takes::HalfOpen, 0, 2, nullptr,
     [](FilterArgs& a, const Value& v) { a.tonemapSaturation = v.x; }, "--tonemap-saturation takes a finite number in (0, 2]",
     kTonemapElsewhere},
    {"--residual-weight", "the weight of the out-of-span layer (nle::DetailOptions of enhance / toneMap)", kEnhance, Takes::Finite, 0, 0,
     nullptr, [](FilterArgs& a, const Value& v) { a.detail.residualWeight = v.x; }, "--residual-weight takes a finite number",
     kDetailElsewhere},
    {"--detail-gain", "the detail curve's gain below --detail-sigma (nle::DetailOptions)", kEnhance, Takes::Closed, 0, NLE_DETAIL_GAIN_MAX,
     nullptr, [](FilterArgs& a, const Value& v) { a.detail.gain = v.x; },
     "--detail-gain takes a finite number in [0, " NLECLI_STR(NLE_DETAIL_GAIN_MAX) "]", kDetailElsewhere},
    {"--detail-sigma", "the amplitude the detail curve's gain acts below (nle::DetailOptions)", kEnhance, Takes::NonNegative, 0, 0, nullptr,
     [](FilterArgs& a, const Value& v) { a.detail.sigma = v.x; }, "--detail-sigma takes a finite number >= 0", kDetailElsewhere},
    {"--shadows", "the base tone curve's slope at its dark end is 1 + S (nle::ToneOptions of enhance)", kEnhance, Takes::Closed, -1, 1,
     nullptr, [](FilterArgs& a, const Value& v) { a.tone.shadows = v.x; }, "--shadows takes a finite number in [-1, 1]", kToneElsewhere},
    {"--highlights", "the base tone curve's slope at its bright end is 1 + Hh (nle::ToneOptions)", kEnhance, Takes::Closed, -1, 1, nullptr,
     [](FilterArgs& a, const Value& v) { a.tone.highlights = v.x; }, "--highlights takes a finite number in [-1, 1]", kToneElsewhere},
    {"--auto-levels", "the base tone curve spans what is left of the base layer when P percent are clipped at either end "
                      "(nle::ToneOptions::clipPercent)",
     kEnhance, Takes::Closed, 0, 25, nullptr, [](FilterArgs& a, const Value& v) { a.tone.clipPercent = v.x, a.toneLine = true; },
     "--auto-levels takes a finite number in [0, 25]", kToneElsewhere},
    {"--equalise", "the share of histogram equalisation in the base tone curve (nle::ToneOptions)", kEnhance, Takes::Closed, 0, 1, nullptr,
     [](FilterArgs& a, const Value& v) { a.tone.equalise = v.x, a.toneLine = true; }, "--equalise takes a finite number in [0, 1]",
     kToneElsewhere},
    {"--segments", "automatic regions (NLEFilter::segment): C segments proposed by the trained filter; two more kinds of stdout line",
     kEnhance, Takes::Integer, 2, NLE_REGION_MAX, nullptr, [](FilterArgs& a, const Value& v) { a.segments = (int)v.x; },
     "--segments takes an integer in [2, " NLECLI_STR(NLE_REGION_MAX) "]", kSegmentElsewhere},
    {"--segment-spread", "how far a segment's indicator spreads (nle::SegmentOptions::spread)", kEnhance, Takes::Positive, 0, 0, nullptr,
     [](FilterArgs& a, const Value& v) { a.segmentSpread = v.x; }, "--segment-spread takes a finite number > 0", kSegmentElsewhere},
    {"--segment-iterations", "the cap on the iterations (nle::SegmentOptions::maxIterations)", kEnhance, Takes::Integer, 1,
     NLE_SEGMENT_ITERATIONS_MAX, nullptr, [](FilterArgs& a, const Value& v) { a.segmentIterations = (int)v.x; },
     "--segment-iterations takes an integer in [1, " NLECLI_STR(NLE_SEGMENT_ITERATIONS_MAX) "]", kSegmentElsewhere},
    {"--segment-map", "the labels as an 8-bit grey image, segment c at round(255 c / (C - 1)), written to FILE", kEnhance, Takes::FileName,
     0, 0, nullptr, [](FilterArgs& a, const Value& v) { a.segmentMap = v.text; }, "--segment-map takes a file name", kSegmentElsewhere},
    {"--segment-weights", "the layer weights of segment c (NLEFilter::enhanceSegments): as many as positional ones, which every other "
                          "segment keeps; once per segment",
     kEnhance, Takes::SegmentWeights, 0, NLE_REGION_MAX - 1, nullptr,
     [](FilterArgs& a, const Value& v) { a.segmentWeights.push_back(v.region), a.segmentOf.push_back((int)v.x); },
     "--segment-weights takes c:w1,w2,... (a segment number and finite weights)", kSegmentElsewhere},
    {"--local", "a local adjustment (NLEFilter::enhanceLocal / enhanceSegmentsLocal): TARGET is a mask as --region takes it, or @c, "
                "segment c of --segments C; the keys are weights=w1/w2/... (as many as positional ones), residual, gain, sigma, "
                "shadows, highlights and saturation, each at most once; a key not named is the background's, which is the "
                "positional weights, --residual-weight, --detail-gain, --detail-sigma, --shadows, --highlights and --saturation; up "
                "to NLE_REGION_MAX times",
     kEnhance, Takes::Local, 0, 0, nullptr, [](FilterArgs& a, const Value& v) { a.locals.push_back(v.local); },
     "--local takes TARGET:key=value[,key=value...] (a mask or @c, then at least one key)", kLocalElsewhere},
    {"--saturation", "the background's saturation of a and b about 128 in a local adjustment (nle::LocalEdit::saturation)", kEnhance,
     Takes::Closed, 0, NLE_LOCAL_SATURATION_MAX, nullptr, [](FilterArgs& a, const Value& v) { a.saturation = v.x; },
     "--saturation takes a finite number in [0, " NLECLI_STR(NLE_LOCAL_SATURATION_MAX) "]", kLocalElsewhere},
    {"--local-auto", "auto levels and equalisation for one row of a local adjustment, on the row's own membership-weighted histogram "
                     "(nle::LocalEdit::clipPercent, equalise): ROW is 0 for the background and m for the m-th --local; levels=P clips "
                     "P percent at either end, equalise=A is the share of histogram equalisation; at least one of the two; once per "
                     "row; one more stdout line per row",
     kEnhance, Takes::LocalAuto, 0, NLE_REGION_MAX, nullptr, [](FilterArgs& a, const Value& v) { a.localAutos.push_back(v.localAuto); },
     "--local-auto takes ROW:levels=P[,equalise=A] (a row number, then at least one of the two keys)", kLocalElsewhere},
    {"--prefilter", "the pre-filter of the MSE-guided denoiser (nle::DenoiseOptions)", kDenoise, Takes::Word, 0, 0, kPrefilters,
     [](FilterArgs& a, const Value& v) { a.denoise.prefilter = (int)v.x; }, "--prefilter takes 'bilateral' or 'nlm'", kDenoiseElsewhere},
    {"--glide", "shrink every plane by the power the MSE estimate picks; the positional shrink factor is the upper end of the search",
     kDenoise, Takes::Flag, 0, 0, nullptr, [](FilterArgs& a, const Value&) { a.denoise.glide = true; }, "--glide takes no value",
     kDenoiseElsewhere},
    {"--noise-sigma", "the noise level of every plane, in place of the estimate", kDenoise, Takes::NonNegative, 0, 0, nullptr,
     [](FilterArgs& a, const Value& v) { a.denoise.noiseSigma = v.x; }, "--noise-sigma takes a finite number >= 0", kDenoiseElsewhere},
    {"--nlm-h", "the NLM pre-filter's h, in place of the table's", kDenoise, Takes::Positive, 0, 0, nullptr,
     [](FilterArgs& a, const Value& v) { a.denoise.nlmH = v.x; }, "--nlm-h takes a finite number > 0", kDenoiseElsewhere},
};

// every refusal: one line on stderr, status 2
[[noreturn]] inline void refuse(const char* prog, const std::string& text) {
    std::cerr << prog << ": " << text << std::endl;
    std::exit(2);
}

// the row that claims `word`: its name, a flag's `name=...`, or any other word that starts with a FlagAnySuffix name
inline const Option* find_option(const std::string& word) {
    for (const Option& o : kOptions)
        if (word == o.name) return &o;
    for (const Option& o : kOptions) {
        if (o.takes == Takes::Flag && word.rfind(std::string(o.name) + "=", 0) == 0) return &o;
        if (o.takes == Takes::FlagAnySuffix && word.rfind(o.name, 0) == 0) return &o;
    }
    return nullptr;
}

// the whole of `v` as a number the row takes
inline bool number(const Option& o, const std::string& v, double* x) {
    char* end = nullptr;
    if (o.takes == Takes::Integer) {
        const long r = v.empty() ? -1 : std::strtol(v.c_str(), &end, 10);
        *x = (double)r;
        return !v.empty() && *end == '\0' && r >= o.lo && r <= o.hi;
    }
    *x = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
    if (v.empty() || *end != '\0' || !std::isfinite(*x)) return false;
    switch (o.takes) {
        case Takes::Positive: return *x > 0;
        case Takes::NonNegative: return !(*x < 0);
        case Takes::Closed: return !(*x < o.lo || *x > o.hi);
        case Takes::HalfOpen: return *x > o.lo && !(*x > o.hi);
        default: return true;
    }
}

// MASK:w1,w2,... split at the last `:`
inline bool region(const std::string& v, FilterArgs::Region* r) {
    static const Option weight = {"", "", 0, Takes::Finite, 0, 0, nullptr, nullptr, "", ""};
    const size_t colon = v.rfind(':');
    if (colon == std::string::npos || colon == 0 || colon + 1 >= v.size()) return false;
    r->mask = v.substr(0, colon);
    const std::string list = v.substr(colon + 1) + ",";
    for (size_t p = 0, q; (q = list.find(',', p)) != std::string::npos; p = q + 1) {
        double x;
        if (!number(weight, list.substr(p, q - p), &x)) return false;
        r->weights.push_back(x);
    }
    return true;
}

// the keys of --local, in the order of FilterArgs::Local::given; `takes` says what the value is (entry 0: a list)
struct LocalKey {
    const char* name;
    Takes takes;
    double lo, hi;
    const char* takesText;
};
inline const LocalKey kLocalKeys[] = {
    {"weights", Takes::Finite, 0, 0, "finite numbers w1/w2/..."},
    {"residual", Takes::Finite, 0, 0, "a finite number"},
    {"gain", Takes::Closed, 0, NLE_DETAIL_GAIN_MAX, "a finite number in [0, " NLECLI_STR(NLE_DETAIL_GAIN_MAX) "]"},
    {"sigma", Takes::NonNegative, 0, 0, "a finite number >= 0"},
    {"shadows", Takes::Closed, -1, 1, "a finite number in [-1, 1]"},
    {"highlights", Takes::Closed, -1, 1, "a finite number in [-1, 1]"},
    {"saturation", Takes::Closed, 0, NLE_LOCAL_SATURATION_MAX, "a finite number in [0, " NLECLI_STR(NLE_LOCAL_SATURATION_MAX) "]"},
};
constexpr int kLocalKeyCount = (int)(sizeof(kLocalKeys) / sizeof(kLocalKeys[0]));
enum { kLocalWeights = 0, kLocalResidual, kLocalGain, kLocalSigma, kLocalShadows, kLocalHighlights, kLocalSaturation };

// TARGET:key=value[,key=value...] split at the last `:`.  False with *why empty: the shape is wrong (the row's own text
// says what it takes); false with *why set: what is wrong inside the spec
inline bool local(const std::string& v, FilterArgs::Local* r, std::string* why) {
    const size_t colon = v.rfind(':');
    if (colon == std::string::npos || colon == 0 || colon + 1 >= v.size()) return false;
    r->target = v.substr(0, colon);
    if (r->target[0] == '@') {
        const Option segment = {"", "", 0, Takes::Integer, 0, NLE_REGION_MAX - 1, nullptr, nullptr, "", ""};
        double c;
        if (!number(segment, r->target.substr(1), &c)) {
            *why = "a segment target is @c with c a whole number in [0, " + std::to_string(NLE_REGION_MAX - 1) + "]";
            return false;
        }
        r->segment = (int)c;
    }
    const std::string list = v.substr(colon + 1) + ",";
    for (size_t p = 0, q; (q = list.find(',', p)) != std::string::npos; p = q + 1) {
        const std::string item = list.substr(p, q - p);
        const size_t eq = item.find('=');
        if (eq == std::string::npos || eq == 0) return false;
        const std::string key = item.substr(0, eq), val = item.substr(eq + 1);
        int k = 0;
        while (k < kLocalKeyCount && key != kLocalKeys[k].name) ++k;
        if (k == kLocalKeyCount) {
            *why = "unknown key '" + key + "' (the keys are weights, residual, gain, sigma, shadows, highlights, saturation)";
            return false;
        }
        if (r->given[k]) {
            *why = "key '" + key + "' is given twice";
            return false;
        }
        r->given[k] = true;
        const Option one = {"", "", 0, kLocalKeys[k].takes, kLocalKeys[k].lo, kLocalKeys[k].hi, nullptr, nullptr, "", ""};
        bool ok = true;
        if (k == kLocalWeights) {
            const std::string ws = val + "/";
            for (size_t a = 0, b; ok && (b = ws.find('/', a)) != std::string::npos; a = b + 1) {
                double x;
                ok = number(one, ws.substr(a, b - a), &x);
                r->weights.push_back(x);
            }
        } else {
            ok = number(one, val, &r->value[k]);
        }
        if (!ok) {
            *why = key + " takes " + kLocalKeys[k].takesText + ", got '" + val + "'";
            return false;
        }
    }
    return true;
}

// ROW:levels=P[,equalise=A] split at the first `:`; false and *why as for local()
inline bool local_auto(const Option& o, const std::string& v, FilterArgs::LocalAuto* r, std::string* why) {
    const size_t colon = v.find(':');
    if (colon == std::string::npos || colon == 0 || colon + 1 >= v.size()) return false;
    r->text = v;
    const Option rowTakes = {"", "", 0, Takes::Integer, o.lo, o.hi, nullptr, nullptr, "", ""};
    double row;
    if (!number(rowTakes, v.substr(0, colon), &row)) {
        *why = "a row is a whole number in [0, " + std::to_string((int)o.hi) + "], 0 the background and m the m-th --local";
        return false;
    }
    r->row = (int)row;
    const Option levels = {"", "", 0, Takes::Closed, 0, 25, nullptr, nullptr, "", ""}, equalise = {"", "", 0, Takes::Closed, 0, 1, nullptr, nullptr, "", ""};
    const std::string list = v.substr(colon + 1) + ",";
    for (size_t p = 0, q; (q = list.find(',', p)) != std::string::npos; p = q + 1) {
        const std::string item = list.substr(p, q - p);
        const size_t eq = item.find('=');
        if (eq == std::string::npos || eq == 0) return false;
        const std::string key = item.substr(0, eq), val = item.substr(eq + 1);
        const bool isLevels = key == "levels";
        if (!isLevels && key != "equalise") {
            *why = "unknown key '" + key + "' (the keys are levels, equalise)";
            return false;
        }
        bool& has = isLevels ? r->hasLevels : r->hasEqualise;
        if (has) {
            *why = "key '" + key + "' is given twice";
            return false;
        }
        has = true;
        if (!number(isLevels ? levels : equalise, val, isLevels ? &r->levels : &r->equalise)) {
            *why = key + " takes a finite number in " + (isLevels ? "[0, 25]" : "[0, 1]") + ", got '" + val + "'";
            return false;
        }
    }
    return true;
}

// the row of the local adjustment's combine that --local-auto's ROW names: masks are rows in the order given, a segment
// target @c is row c + 1
inline int local_auto_row(const FilterArgs& a, const FilterArgs::LocalAuto& u) {
    if (u.row == 0) return 0;
    const FilterArgs::Local& l = a.locals[(size_t)u.row - 1];
    return l.segment >= 0 ? l.segment + 1 : u.row;
}

// row `l` of a local adjustment (null: the background's row) as the C++ surface takes it: what the spec names, and the
// background's for every key it does not
inline nle::LocalEdit local_edit(const FilterArgs& a, const FilterArgs::Local* l) {
    nle::LocalEdit e;
    e.weights = a.extra;
    e.detail = a.detail;
    e.shadows = a.tone.shadows, e.highlights = a.tone.highlights, e.saturation = a.saturation;
    if (!l) return e;
    if (l->given[kLocalWeights]) e.weights = l->weights;
    if (l->given[kLocalResidual]) e.detail.residualWeight = l->value[kLocalResidual];
    if (l->given[kLocalGain]) e.detail.gain = l->value[kLocalGain];
    if (l->given[kLocalSigma]) e.detail.sigma = l->value[kLocalSigma];
    if (l->given[kLocalShadows]) e.shadows = l->value[kLocalShadows];
    if (l->given[kLocalHighlights]) e.highlights = l->value[kLocalHighlights];
    if (l->given[kLocalSaturation]) e.saturation = l->value[kLocalSaturation];
    return e;
}

// the same with the row's --local-auto, if it has one; row: 0 the background, m the m-th --local
inline nle::LocalEdit local_edit_row(const FilterArgs& a, int row) {
    nle::LocalEdit e = local_edit(a, row == 0 ? nullptr : &a.locals[(size_t)row - 1]);
    for (const auto& u : a.localAutos)
        if (u.row == row) e.clipPercent = u.hasLevels ? u.levels : -1, e.equalise = u.hasEqualise ? u.equalise : 0;
    return e;
}

// false (after printing the usage line to stderr) when fewer than `min_argc` arguments were given
inline bool parse(int argc, char* argv[], int min_argc, FilterArgs* a, Tool tool) {
    const char* prog = argv[0];
    std::vector<char*> shifted;
    std::vector<const Option*> given;  // the options read, in their order
    int first = 1;                     // the first argument after the leading options
    while (first < argc) {
        const std::string word = argv[first];
        const Option* o = find_option(word);
        if (!o) break;
        if (!(o->tools & (int)tool))
            refuse(prog, (o->elsewhereSaysName ? o->name : word) + " is not supported here: " + o->elsewhereText);
        const bool flag = o->takes == Takes::Flag || o->takes == Takes::FlagAnySuffix;
        Value v;
        v.text = flag ? word : first + 1 < argc ? argv[first + 1] : "";
        std::string got = v.text;
        bool ok = false;
        switch (o->takes) {
            case Takes::Flag:
            case Takes::FlagAnySuffix: ok = word == o->name; break;
            case Takes::Word:
                for (const Word* w = o->words; w->word && !ok; ++w)
                    if (v.text == w->word) v.x = w->value, ok = true;
                break;
            case Takes::FileName:
                ok = !v.text.empty() && v.text.rfind("--", 0) != 0;
                got = word + " " + v.text;
                break;
            case Takes::Region: ok = region(v.text, &v.region); break;
            case Takes::SegmentWeights: {
                const Option segment = {"", "", 0, Takes::Integer, o->lo, o->hi, nullptr, nullptr, "", ""};
                ok = region(v.text, &v.region) && number(segment, v.region.mask, &v.x);
                break;
            }
            case Takes::Local: {
                std::string why;
                ok = local(v.text, &v.local, &why);
                if (!ok && !why.empty()) refuse(prog, "--local " + v.text + ": " + why);
                break;
            }
            case Takes::LocalAuto: {
                std::string why;
                ok = local_auto(*o, v.text, &v.localAuto, &why);
                if (!ok && !why.empty()) refuse(prog, "--local-auto " + v.text + ": " + why);
                break;
            }
            default: ok = number(*o, v.text, &v.x);
        }
        if (!ok) refuse(prog, std::string(o->takesText) + ", got '" + got + "'");
        if (o->takes == Takes::Local && (int)a->locals.size() == NLE_REGION_MAX)
            refuse(prog, "--local can be given at most " NLECLI_STR(NLE_REGION_MAX) " times");
        if (o->takes == Takes::Region && (int)a->regions.size() == NLE_REGION_MAX)
            refuse(prog, "--region can be given at most " NLECLI_STR(NLE_REGION_MAX) " times");
        o->set(*a, v);
        given.push_back(o);
        first += flag ? 1 : 2;
    }
    // the name of the last option given among `names`, "" if none was
    const auto last = [&](std::initializer_list<const char*> names) {
        for (auto g = given.rbegin(); g != given.rend(); ++g)
            for (const char* n : names)
                if (std::string((*g)->name) == n) return std::string(n);
        return std::string();
    };
    const auto is_given = [&](const char* name) { return !last({name}).empty(); };
    // what holds between options, in the order the refusals have
    if (is_given("--noise-sigma") && !a->denoise.glide && a->denoise.prefilter != NLE_PREFILTER_NLM)
        refuse(prog, "--noise-sigma needs --glide or --prefilter nlm (nothing else uses a noise level)");
    if (is_given("--nlm-h") && a->denoise.prefilter != NLE_PREFILTER_NLM) refuse(prog, "--nlm-h needs --prefilter nlm");
    if (a->exact && (a->patchRadius != 0 || a->sampler != NLE_SAMPLER_GRID))
        refuse(prog, "--exact uses no samples and single-pixel affinities: it does not combine with --patch-radius R > 0, "
                     "--sampler farthest or --sampler residual");
    if (a->chroma != 0 && (a->exact || a->patchRadius > NLE_CHROMA_PATCH_RADIUS_MAX))
        refuse(prog, "--chroma does not combine with --exact or with --patch-radius R > " NLECLI_STR(NLE_CHROMA_PATCH_RADIUS_MAX));
    if (!a->nystromMap.empty() && !a->nystromReport) refuse(prog, "--nystrom-map needs --nystrom-report");
    if (a->nystromReport && a->exact)
        refuse(prog, "--nystrom-report and --nystrom-map do not combine with --exact: the exact filter has no Nystrom extension");
    if (a->deep && !a->regions.empty()) refuse(prog, "--deep does not combine with --region: region edits take an 8-bit image");
    if (is_given("--tonemap-saturation") && !a->tonemap) refuse(prog, "--tonemap-saturation needs --tonemap");
    if (a->tonemap && (a->chroma != 0 || !a->regions.empty() || a->deep || a->nystromReport))
        refuse(prog, "--tonemap does not combine with --chroma, --region, --deep or --nystrom-report: those take an 8-bit or "
                     "16-bit sRGB image");
    if (a->detail.gain != 1 && !(a->detail.sigma > 0))
        refuse(prog, "--detail-gain other than 1 needs --detail-sigma S > 0 (the amplitude the gain acts below)");
    const std::string detailGiven = last({"--residual-weight", "--detail-gain", "--detail-sigma"});
    if (!detailGiven.empty() && !a->regions.empty())
        refuse(prog, detailGiven + " does not combine with --region: region edits have no residual layer and no detail curve");
    const std::string toneGiven = last({"--shadows", "--highlights", "--auto-levels", "--equalise"});
    if (!toneGiven.empty() && (!a->regions.empty() || a->tonemap))
        refuse(prog, toneGiven + " does not combine with --region or --tonemap: the base tone curve is built for the plain 8-bit and "
                                 "16-bit enhance");
    // local adjustments: what --local does not combine with, then its targets
    bool localMasks = false, localSegments = false;
    for (const auto& l : a->locals) (l.segment < 0 ? localMasks : localSegments) = true;
    if (is_given("--saturation") && a->locals.empty())
        refuse(prog, "--saturation needs --local (it is the background's saturation in a local adjustment)");
    if (!a->locals.empty()) {
        if (!a->regions.empty() || !a->segmentWeights.empty() || a->tonemap || is_given("--auto-levels") || is_given("--equalise"))
            refuse(prog, "--local does not combine with --region, --segment-weights, --tonemap, --auto-levels or --equalise: a region "
                         "has one kind of edit, and a whole-image histogram has no per-region meaning yet");
        if (localMasks && localSegments)
            refuse(prog, "--local targets are all masks or all segments (@c), got both");
        if (localSegments && a->segments == 0) refuse(prog, "--local @c needs --segments C");
        if (localMasks && a->segments != 0)
            refuse(prog, "--local with a mask does not combine with --segments: the segments are targeted as @c");
        for (size_t k = 0; k < a->locals.size(); ++k) {
            const auto& l = a->locals[k];
            if (l.segment >= a->segments && l.segment >= 0)
                refuse(prog, "--local " + l.target + ": there are " + std::to_string(a->segments) + " segments, numbered from 0");
            for (size_t j = 0; j < k; ++j)
                if (l.segment >= 0 && a->locals[j].segment == l.segment)
                    refuse(prog, "--local can be given once per segment, segment " + std::to_string(l.segment) + " has two");
            const nle::LocalEdit e = local_edit(*a, &l);
            if (e.detail.gain != 1 && !(e.detail.sigma > 0))
                refuse(prog, "--local " + l.target + ": a gain other than 1 needs a sigma > 0, its own or --detail-sigma's");
        }
    }
    if (!a->localAutos.empty() && a->locals.empty())
        refuse(prog, "--local-auto needs at least one --local (ROW 0 is its background, ROW m the m-th --local)");
    for (size_t k = 0; k < a->localAutos.size(); ++k) {
        const auto& u = a->localAutos[k];
        if (u.row > (int)a->locals.size())
            refuse(prog, "--local-auto " + u.text + ": there are " + std::to_string(a->locals.size() + 1) +
                             " rows, 0 the background and m the m-th --local");
        for (size_t j = 0; j < k; ++j)
            if (a->localAutos[j].row == u.row)
                refuse(prog, "--local-auto can be given once per row, row " + std::to_string(u.row) + " has two");
    }
    if ((is_given("--region-spread") || is_given("--region-floor")) && a->regions.empty() && !localMasks)
        refuse(prog, "--region-spread and --region-floor need at least one --region");
    const std::string segmentGiven = last({"--segment-spread", "--segment-iterations", "--segment-map", "--segment-weights"});
    if (!segmentGiven.empty() && a->segments == 0) refuse(prog, segmentGiven + " needs --segments C");
    if (a->segments != 0) {
        if (!a->regions.empty() || a->deep || a->tonemap)
            refuse(prog, "--segments does not combine with --region, --deep or --tonemap: the segments are the regions of an 8-bit "
                         "region edit");
        if ((!detailGiven.empty() || !toneGiven.empty()) && a->locals.empty())  // (with --local they are the background's row)
            refuse(prog, (detailGiven.empty() ? toneGiven : detailGiven) +
                             " does not combine with --segments: region edits have no residual layer, no detail curve and no tone curve");
        for (size_t k = 0; k < a->segmentOf.size(); ++k) {
            if (a->segmentOf[k] >= a->segments)
                refuse(prog, "--segment-weights " + a->segmentWeights[k].mask + ": there are " + std::to_string(a->segments) +
                                 " segments, numbered from 0");
            for (size_t j = 0; j < k; ++j)
                if (a->segmentOf[j] == a->segmentOf[k])
                    refuse(prog, "--segment-weights can be given once per segment, segment " + std::to_string(a->segmentOf[k]) +
                                     " has two");
        }
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
        if (ext != ".png")
            refuse(prog, std::string(a->deep ? "--deep" : "--tonemap") + " writes a 16-bit PNG: the output name must end in .png, got '" +
                             o + "'");
    }
    int* ints[] = {&a->rowSamples, &a->colSamples, nullptr, nullptr, &a->sinkhornIters, &a->eigenVectors};
    double* reals[] = {nullptr, nullptr, &a->hx, &a->hy, nullptr, nullptr};
    for (int i = 0; i < 6; ++i) {
        if (ints[i]) *ints[i] = std::stoi(argv[3 + i]);
        else *reals[i] = std::stod(argv[3 + i]);
    }
    for (int i = 9; i < argc; ++i) a->extra.push_back(std::stod(argv[i]));
    const std::string most = " takes at most " NLECLI_STR(NLE_REGION_LAYERS_MAX) " weights, got " + std::to_string(a->extra.size());
    if (a->detail.active() && (int)a->extra.size() > NLE_REGION_LAYERS_MAX) refuse(prog, detailGiven + most);
    if (a->tone.active() && (int)a->extra.size() > NLE_REGION_LAYERS_MAX) refuse(prog, toneGiven + most);
    if (!a->regions.empty()) {  // every region has the background's weight count
        if ((int)a->extra.size() > NLE_REGION_LAYERS_MAX) refuse(prog, "--region" + most);
        for (const auto& r : a->regions)
            if (r.weights.size() != a->extra.size())
                refuse(prog, "--region " + r.mask + " has " + std::to_string(r.weights.size()) + " weights, the command line has " +
                                 std::to_string(a->extra.size()));
    }
    if (!a->locals.empty()) {  // every row that names weights has the positional weight count
        if ((int)a->extra.size() > NLE_REGION_LAYERS_MAX) refuse(prog, "--local" + most);
        for (const auto& l : a->locals)
            if (l.given[kLocalWeights] && l.weights.size() != a->extra.size())
                refuse(prog, "--local " + l.target + " has " + std::to_string(l.weights.size()) + " weights, the command line has " +
                                 std::to_string(a->extra.size()));
    }
    if (!a->segmentWeights.empty()) {  // every segment has the positional weight count
        if ((int)a->extra.size() > NLE_REGION_LAYERS_MAX) refuse(prog, "--segment-weights" + most);
        for (const auto& r : a->segmentWeights)
            if (r.weights.size() != a->extra.size())
                refuse(prog, "--segment-weights " + r.mask + " has " + std::to_string(r.weights.size()) +
                                 " weights, the command line has " + std::to_string(a->extra.size()));
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
