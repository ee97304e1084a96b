// The host-mediated all-reduce of a device group whose ranks are threads of one process: a barrier, one slot per rank
// and a sum in rank order, so that every rank ends with bitwise the same sums.  Owns nothing else: no GPU, no nle.h --
// it compiles and runs on its own (tools/micro/rank_sum_check.cpp drives it under ThreadSanitizer).
#pragma once

#include <condition_variable>
#include <cstddef>
#include <mutex>
#include <stdexcept>
#include <vector>

namespace nle {

class RankSum {
public:
    explicit RankSum(int ranks) : slot_((size_t)ranks, nullptr), acc_((size_t)ranks) {}
    int size() const { return (int)slot_.size(); }

    // v[0..n) becomes the sum over the ranks of their v, added as 0 + slot 0 + slot 1 + ... on every rank; every rank
    // of the group calls it with the same n.  Throws once the group has failed, also while it waits for the others.
    void sum(int rank, double* v, size_t n) {
        slot_[(size_t)rank] = v;
        barrier();  // every slot is filled
        std::vector<double>& acc = acc_[(size_t)rank];
        acc.assign(n, 0.0);
        for (const double* s : slot_)  // rank order: identical on every rank
            for (size_t i = 0; i < n; ++i) acc[i] += s[i];
        barrier();  // every rank has read every slot
        for (size_t i = 0; i < n; ++i) v[i] = acc[i];
    }

    // a rank that will not arrive says so: every rank waiting in sum(), and every later sum(), throws
    void fail() {
        std::lock_guard<std::mutex> lk(mu_);
        failed_ = true;
        cv_.notify_all();
    }
    bool failed() const {
        std::lock_guard<std::mutex> lk(mu_);
        return failed_;
    }
    // after a failed round, once no rank is inside sum() any more: the next round starts clean
    void recover() {
        std::lock_guard<std::mutex> lk(mu_);
        failed_ = false;
        arrived_ = 0;
    }

private:
    void barrier() {
        std::unique_lock<std::mutex> lk(mu_);
        if (failed_) throw std::runtime_error("nle: another rank of the device group failed");
        const long long gen = generation_;
        if (++arrived_ == size()) {
            arrived_ = 0;
            ++generation_;
            cv_.notify_all();
        } else {
            cv_.wait(lk, [&] { return generation_ != gen || failed_; });
            if (failed_) throw std::runtime_error("nle: another rank of the device group failed");
        }
    }

    mutable std::mutex mu_;
    std::condition_variable cv_;
    int arrived_ = 0;
    long long generation_ = 0;
    bool failed_ = false;
    std::vector<const double*> slot_;       // one per rank: the rank's own buffer, read between the two barriers
    std::vector<std::vector<double>> acc_;  // one per rank, kept between rounds
};

}  // namespace nle
