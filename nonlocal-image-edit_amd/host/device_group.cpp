// The NLE_DEVICES device group (device_group.hpp): parsing the list, one ctx per device, binding the library's RCCL
// communicator or the host-mediated all-reduce callback to every rank.
#include "device_group.hpp"

#include <algorithm>
#include <cstdlib>
#include <sstream>
#include <string>

#include "nle.h"
#include "surface_internal.hpp"

namespace nle::surface {

const char* devices_env() { return std::getenv("NLE_DEVICES"); }

DeviceGroup::DeviceGroup(const std::vector<int>& devices)
    : devs(devices), ctx(devices.size(), nullptr), sums((int)devices.size()), d_comm(devices.size(), nullptr),
      ranks(devices.size()) {
    std::vector<int> sorted(devs);
    std::sort(sorted.begin(), sorted.end());
    native = std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
    for (int r = 0; r < size(); ++r) {
        if (nle_ctx_create(devs[r], nullptr, &ctx[r]) != NLE_OK)
            throw std::runtime_error(std::string("nle: cannot create GPU context: ") + nle_last_error(nullptr));
        nle_ctx_set_mode(ctx[r], default_mode());
        ranks[r].g = this;
        ranks[r].r = r;
    }
}

void DeviceGroup::fail() {
    sums.fail();  // ranks waiting in the host-mediated all-reduce
    // ranks waiting in a native collective for the one that failed: abort every communicator of the group, their
    // pending ncclAllReduce ends and their next call returns NLE_ERR_COMM; device_group() rebuilds the group (a fresh
    // unique id, ncclCommInitRank on every ctx) before the next train
    if (native)
        for (nle_ctx* c : ctx)
            if (c) (void)nle_ctx_abort_rccl(c);
}

void DeviceGroup::recover() {
    sums.recover();
    bound_p = -1;
    native_bound = false;
}

int DeviceGroup::allreduce_cb(void* user, void* d_buf, size_t count) {
    Rank* me = static_cast<Rank*>(user);
    nle_ctx* c = me->g->ctx[me->r];
    try {
        me->buf.resize(count);
        if (nle_dev_download(c, me->buf.data(), d_buf, count * sizeof(double)) != NLE_OK) return 1;
        me->g->sums.sum(me->r, me->buf.data(), count);
        return nle_dev_upload(c, d_buf, me->buf.data(), count * sizeof(double)) == NLE_OK ? 0 : 1;
    } catch (...) {
        return 1;
    }
}

DeviceGroup* device_group(int p_samples) {
    static DeviceGroup* g = nullptr;
    static bool looked = false;
    if (!looked) {
        looked = true;
        const char* e = devices_env();
        std::istringstream list(e ? e : "");
        std::vector<int> devs;
        for (std::string tok; std::getline(list, tok, ',');)
            if (!tok.empty()) devs.push_back(std::stoi(tok));
        if (devs.size() >= 2) g = new DeviceGroup(devs);
    }
    if (g && p_samples > 0) {
        if (g->sums.failed()) g->recover();  // an earlier train / enhance of this process failed on some rank
        // (re)bind the communicator for this sample count: the callback form needs a comm buffer of nle_comm_len(p)
        if (g->bound_p != p_samples) {
            const int G = g->size();
            if (g->native) {
                if (!g->native_bound) {
                    unsigned char id[NLE_RCCL_UNIQUE_ID_BYTES];
                    check(nle_rccl_unique_id(id, sizeof id), nullptr);
                    g->run([&](int r) { check(nle_ctx_init_rccl(g->ctx[r], r, G, id, sizeof id), g->ctx[r]); });
                    g->native_bound = true;
                }
            } else {
                const size_t len = nle_comm_len(p_samples);
                for (int r = 0; r < G; ++r) {
                    if (g->d_comm[r]) nle_dev_free(g->ctx[r], g->d_comm[r]);
                    check(nle_dev_alloc(g->ctx[r], len * sizeof(double), &g->d_comm[r]), g->ctx[r]);
                    check(nle_ctx_set_shard(g->ctx[r], r, G, &DeviceGroup::allreduce_cb, &g->ranks[r],
                                            static_cast<double*>(g->d_comm[r]), len), g->ctx[r]);
                }
            }
            for (int r = 0; r < G; ++r) check(nle_ctx_set_slab_input(g->ctx[r], 1), g->ctx[r]);
            g->bound_p = p_samples;
        }
    }
    return g;
}

}  // namespace nle::surface
