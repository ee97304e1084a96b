// The sample set and the fp64 affinity rows on the host: what an affinity is on the fp64 formulations -- the patch radius
// (nle_ctx_set_patch_radius), the chroma planes (nle_ctx_set_chroma) and the sampler (nle_ctx_set_sampler) -- is read from
// the ctx, refused, fetched, turned into Ka and into row launches HERE (samples.hip); the train paths and stage entry points
// (train.h) see an AffinityOpts, a SampleSet and an AffinityRows64.  Not installed, not part of the ABI.
#pragma once
#include "pipeline_internal.h"

namespace nlep {

// The ctx's affinity options, read once (affinity_opts): nothing else reads those fields of the ctx
struct AffinityOpts {
    int R = 0;                  // patch radius: (2R + 1)^2 pixels per patch, 0 = the reference's single-value affinity
    const float* d_a = nullptr; // chroma: the full a and b planes of 8-bit Lab on the device (both null = off) ...
    const float* d_b = nullptr;
    double hc = 0.0;            // ... and the chroma bandwidth
    // NLE_SAMPLER_FARTHEST, NLE_SAMPLER_RESIDUAL: the sample set is a list (sampler.hip), not the grid's closed form
    int sampler = NLE_SAMPLER_GRID;
    bool patch() const { return R > 0; }
    bool chroma() const { return d_a != nullptr; }
    bool listed() const { return sampler != NLE_SAMPLER_GRID; }
    const char* sampler_name() const { return sampler == NLE_SAMPLER_RESIDUAL ? "the residual sampler" : "the farthest sampler"; }
    bool any() const { return patch() || chroma() || listed(); }
    int patch_len() const { return (2 * R + 1) * (2 * R + 1); }
    double cwd() const { return (1.0 / (hc * hc)) / patch_len(); }  // the chroma weight of S_ab: (1/hc^2) / (2R + 1)^2
};
AffinityOpts affinity_opts(const nle_ctx* c);

// Every refusal of the options that needs no device, decided the same way on every rank, for the entry point `where`
// (the fp32 stage entry points take none of the options; nle_sample_pixels looks at the sampler only)
enum class Caller { TRAIN, KERNEL64, KERNEL32, NYSTROM32, SAMPLE_PIXELS };
void check_affinity_opts(const nle_ctx* c, const AffinityOpts& o, const GridSpec& gs, int H, int W, double hx, double hy,
                         Caller where);

struct SampleSet {
    GridSpec gs;
    int p = 0;
    AffinityOpts opts;              // what the set was fetched for (opts.listed(): pix is the sampler's list, not the grid's)
    std::vector<long long> pix;     // row-major pixel index of each sample (permuted order)
    std::vector<float> val;         // luminance
    std::vector<float4> packed;     // {row, col, lum, 0}
    bool quantised = false;         // whole plane integer valued in [0, 255] (checked on request)
    unsigned level_tiles = 0xffffu; // then: which 16-level tiles occur in this rank's part of the plane (bit t)
    std::vector<int> patch;         // R > 0: p x (2R + 1)^2 patch values around each sample (reflect-101), row per sample
    // chroma: the samples' a and b values (R = 0: p each) or patches (R > 0: p x (2R + 1)^2 each, as `patch`)
    std::vector<int> aval, bval;
    bool chroma_quantised = false;  // both chroma planes integer valued in [0, 255]
};

struct FetchSpec {
    bool check_levels = false;  // decide `quantised` and `level_tiles` (always decided with patches or chroma)
    // only this rank's rows exist behind d_lum (a virtual base): values and verdict are completed by an all-reduce; grid only
    bool slab_plane = false;
    const std::vector<long long>* list = nullptr;  // the sample pixels of a listed sampler (ascending, gs.p() of them)
};
// d_lum: base of the full plane.  o.patch(): also the samples' patches; o.chroma(): also their a and b values or patches
// and the level check of the a and b planes
SampleSet fetch_samples(nle_ctx* c, const float* d_lum, const GridSpec& gs, const AffinityOpts& o, const FetchSpec& spec = {});

// The sample pixels of the ctx's listed sampler (NLE_SAMPLER_FARTHEST or NLE_SAMPLER_RESIDUAL, sampler.hip) on the full
// plane d_lum, ascending; the same on every rank.  `order` (one rank, the residual sampler): also the selection as it was made
struct SamplerOrder {
    std::vector<long long> order;  // the samples in the order chosen
    std::vector<double> pivot;     // nle_sample_pixels_order's h_pivot
    int n_residual = 0;
    double stats[3] = {0, 0, 0};
};
std::vector<long long> sampler_list(nle_ctx* c, const float* d_lum, const GridSpec& gs, double hx, double hy,
                                    SamplerOrder* order = nullptr);

// Patches and chroma need integer-valued planes.  agree_over_ranks (train): refused on every rank if a plane is not integer
// valued on one -- one ranks_where per option that is on, patch first
void require_integer_planes(nle_ctx* c, const SampleSet& ss, bool agree_over_ranks);

// Ka(i,j), reference src/filter.cpp:128-137,144 (fp64, integer spatial term), in the kernels' order of operations
std::vector<double> build_Ka(const SampleSet& ss, double hx, double hy);

// the packed samples on the device, zero padded to `padded` entries when that is larger than p
DevBuf<float4> upload_samples(nle_ctx* c, const SampleSet& ss, int padded = 0);

// fp64 affinity rows (natural order, ld4(p) columns) of the plane d_lum under the options of `ss`: everything a launch
// needs on the device.  want_mask: a listed set's bitmask, for rows(.., skip_samples = true)
class AffinityRows64 {
public:
    AffinityRows64(nle_ctx* c, const float* d_lum, const SampleSet& ss, double hx, double hy, bool want_mask);
    // rows [pix0, pix0 + M) into d_kab; skip_samples: the rows of the sample pixels themselves come out as zeros
    hipError_t rows(long long pix0, long long M, double* d_kab, bool skip_samples = false) const {
        return nlek::affinity_rows64(st_, args_, pix0, M, d_kab, skip_samples);
    }

private:
    hipStream_t st_;
    nlek::Affinity64Args args_;
    DevBuf<float4> samples_;
    DevBuf<signed char> spatch_, cpatch_;  // int8 B operands of the patch kernels: L, and a then b
    DevBuf<int> snorm_, cnorm_;
    DevBuf<float2> sab_;                   // chroma at R = 0: the samples' (a, b)
    DevBuf<unsigned> mask_;
};

}  // namespace nlep
