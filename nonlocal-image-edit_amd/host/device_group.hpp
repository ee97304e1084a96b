// NLE_DEVICES=<dev>,<dev>,...  (SURVEY.md section 8e through the reference's own surface): the process's device group.
// One context per listed device, created once per process; rank r owns image rows nle_slab_rows(H, r, G) and hands the
// library only those (nle_ctx_set_slab_input).  All-reduces: the library's own RCCL communicator when the devices are
// distinct (ncclCommInitRank from G threads), otherwise -- the same device listed more than once, a rehearsal on one
// GPU -- the host-mediated sum of rank_sum.hpp, so that every rank sees bitwise the same sums.
#pragma once

#include <exception>
#include <thread>
#include <vector>

#include "rank_sum.hpp"

struct nle_ctx;

namespace nle::surface {

struct DeviceGroup {
    const std::vector<int> devs;
    std::vector<nle_ctx*> ctx;  // one per rank
    bool native = false;        // distinct devices: the library's RCCL communicator
    int bound_p = -1;           // sample count the communicator / comm buffers are bound for (-1: not bound)
    bool native_bound = false;  // the library's RCCL communicator exists on every ctx
    RankSum sums;               // the host-mediated all-reduce
    std::vector<void*> d_comm;
    struct Rank {
        DeviceGroup* g;
        int r;
        std::vector<double> buf;  // the all-reduce's host copy, kept between calls
    };
    std::vector<Rank> ranks;

    explicit DeviceGroup(const std::vector<int>& devices);  // creates the contexts
    int size() const { return (int)devs.size(); }
    // ranks waiting in an all-reduce, host-mediated or native, for a rank that failed: end their wait
    void fail();
    // after a failed run (every rank thread has been joined): forget the failure and whatever was bound, so that the next
    // train binds a fresh communicator / fresh comm buffers instead of failing for the rest of the process
    void recover();
    // nle_allreduce_fn of the host-mediated form: download, RankSum::sum, upload
    static int allreduce_cb(void* user, void* d_buf, size_t count);
    // fn(rank) on one thread per rank; the first exception is rethrown after all threads have ended
    template <typename Fn>
    void run(Fn&& fn) {
        std::vector<std::thread> th;
        std::vector<std::exception_ptr> err(size());
        for (int r = 0; r < size(); ++r)
            th.emplace_back([&, r] {
                try {
                    fn(r);
                } catch (...) {
                    err[r] = std::current_exception();
                    fail();
                }
            });
        for (auto& t : th) t.join();
        for (auto& e : err)
            if (e) std::rethrow_exception(e);
    }
};

// NLE_DEVICES as given (null: unset)
const char* devices_env();

// nullptr unless NLE_DEVICES lists at least two devices; p_samples > 0 (re)binds the group's communicator for that
// sample count (and forgets an earlier failure)
DeviceGroup* device_group(int p_samples);

}  // namespace nle::surface
