// Stand-alone check of host/rank_sum.hpp (the host-mediated all-reduce of a device group), meant to be built with
// -fsanitize=thread; tests/test_rank_sum.py builds and runs it.  No GPU, no library.
//   g++ -std=c++17 -pthread -fsanitize=thread -I nonlocal-image-edit_amd/host tools/micro/rank_sum_check.cpp -o check_rank_sum
// For G in {1, 2, 3, 5} threads and n in {1, 2049} doubles:
//   - 200 back-to-back rounds (the barrier's generation is reused) of values for which the order of addition shows
//     (1e16, 1, -1e16, 3, ...): every rank must end every round with the bits of the sum in rank order;
//   - one round in which one rank calls fail() instead of arriving: every other rank's sum() must throw and every
//     thread must end; after recover() a clean round must succeed.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <vector>

#include "rank_sum.hpp"

static const double kValues[] = {1e16, 1.0, -1e16, 3.0, -2.0, 0.5, 1e16, 7.0, -1e16};
static const int kNValues = sizeof kValues / sizeof kValues[0];

static double contribution(int rank, size_t i, int round) { return kValues[(rank * 2 + (int)(i % 1000) + round) % kNValues]; }

// what every rank must hold after the round: 0 + slot 0 + slot 1 + ...
static double expected(int G, size_t i, int round) {
    double s = 0.0;
    for (int r = 0; r < G; ++r) s += contribution(r, i, round);
    return s;
}

// `rounds` rounds on G threads, starting at round number `first`; returns the number of wrong values and of throws
static void run_rounds(nle::RankSum& rs, int G, size_t n, int first, int rounds, int failing_rank, std::atomic<long>& wrong,
                       std::atomic<int>& threw) {
    std::vector<std::thread> th;
    for (int rank = 0; rank < G; ++rank)
        th.emplace_back([&, rank] {
            std::vector<double> v(n);
            for (int round = first; round < first + rounds; ++round) {
                if (rank == failing_rank) {
                    rs.fail();
                    return;
                }
                for (size_t i = 0; i < n; ++i) v[i] = contribution(rank, i, round);
                try {
                    rs.sum(rank, v.data(), n);
                } catch (const std::runtime_error&) {
                    ++threw;
                    return;
                }
                for (size_t i = 0; i < n; ++i) {
                    const double e = expected(G, i, round);
                    if (std::memcmp(&e, &v[i], sizeof e) != 0) ++wrong;
                }
            }
        });
    for (auto& t : th) t.join();
}

int main() {
    int bad = 0;
    for (int G : {1, 2, 3, 5})
        for (size_t n : {(size_t)1, (size_t)2049}) {
            nle::RankSum rs(G);
            std::atomic<long> wrong{0};
            std::atomic<int> threw{0};
            run_rounds(rs, G, n, 0, 200, -1, wrong, threw);
            const bool sums_ok = wrong == 0 && threw == 0 && !rs.failed();
            // the order must show in these values: the sum in reverse rank order differs somewhere (G >= 3)
            bool order_shows = G < 3;
            for (int round = 0; round < 200 && !order_shows; ++round)
                for (size_t i = 0; i < n && !order_shows; ++i) {
                    double s = 0.0;
                    for (int r = G - 1; r >= 0; --r) s += contribution(r, i, round);
                    order_shows = s != expected(G, i, round);
                }
            // one rank fails instead of arriving: the others throw, nobody hangs
            wrong = 0, threw = 0;
            run_rounds(rs, G, n, 200, 1, G / 2, wrong, threw);
            const bool fail_ok = threw == G - 1 && wrong == 0 && rs.failed();
            bool still_failed = false;  // and the group stays failed until it is recovered
            try {
                double x = 1.0;
                rs.sum(0, &x, 1);
            } catch (const std::runtime_error&) {
                still_failed = true;
            }
            rs.recover();
            wrong = 0, threw = 0;
            run_rounds(rs, G, n, 201, 1, -1, wrong, threw);
            const bool recover_ok = wrong == 0 && threw == 0 && !rs.failed();
            const bool ok = sums_ok && order_shows && fail_ok && still_failed && recover_ok;
            std::printf("G=%d n=%zu: sums %s, order shows %s, failed round %s, stays failed %s, after recover %s\n", G, n,
                        sums_ok ? "ok" : "WRONG", order_shows ? "yes" : "NO", fail_ok ? "ok" : "WRONG",
                        still_failed ? "yes" : "NO", recover_ok ? "ok" : "WRONG");
            bad += !ok;
        }
    std::printf("%s\n", bad == 0 ? "rank_sum_check OK" : "rank_sum_check FAILED");
    return bad == 0 ? 0 : 1;
}
