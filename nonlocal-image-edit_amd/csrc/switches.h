// The library's debugging and measurement switches: one struct, one reader of the process environment.  Nothing else
// under csrc/ asks the environment.  Lifetime: a ctx takes a snapshot when a call on it begins (pipeline_internal.h:
// guard()) and everything below the entry point reads that snapshot; the ctx-less host eigensolver takes its own at
// each public entry (eigen_sym.cpp: read_opts) and hands the two it uses down as an EigOpts.  INTEGRATION.md section 3
// lists the same names for users.  No HIP dependency: eigen_sym.cpp is also compiled stand-alone by a plain C++ compiler.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace nlesw {

// Flags are on when the variable is present, whatever its value (also empty).
struct Switches {
    bool trace = false;              // debug: stage marks and solver notes of a train call on stderr
    bool force_eig = false;          // debug: Ka and Wa by eigendecomposition, never by the Cholesky shortcuts
    bool host_solver = false;        // debug: every p x p solver on the host, whatever the order
    bool host_ka = false;            // debug: the Cholesky factor of Ka on the host
    bool host_wa = false;            // debug: the root of Wa on the host
    bool host_q = false;             // debug: the eigenpairs of Q on the host
    int dev_solver_min = 288;        // measurement: smallest order the device solvers take (clamped to >= 3)
    bool sytrd_g_set = false;        // measurement: sytrd_g below replaces the library's own number of workgroups
    int sytrd_g = 0;                 //   of the persistent Householder reduction (taken as given: <= 0 means host solver)
    bool nystrom_bf16x3 = false;     // measurement: the fused Nystrom GEMM with split bf16 operands (as the ctx setting)
    bool no_sorted_rows = false;     // debug: the table passes on the LDS-atomic kernels, no level-sorted rows
    bool all_level_tiles = false;    // measurement: the table columns of all 16 level tiles, also those that do not occur
    bool sorted_table = false;       // measurement: column factors from the table, neither recurrence nor moment form
    bool sorted_no_moments = false;  // measurement: the pass kernel's pixel loop without the moment form
    bool gram_pairs = false;         // measurement: the Gram in its pair-table form, not on index sums
    int sorted_wgs_per_cu = 2;       // measurement: workgroups per compute unit of the sorted kernels (clamped to >= 1)
    bool auto_stream64 = false;      // debug: auto mode's fp64 fallback always takes the streamed form
    int stream64_chunk_mb = 2048;    // debug: workspace budget of the streamed form's chunk in MiB (clamped to >= 1)
    int q_solver = 0;                // the topk_solver a new ctx starts with: 1 for the value "lanczos", else 0
    bool eig_no_bisect = false;      // measurement: host eigensolver without bisection (QL for all eigenvalues)
    bool eig_no_x8 = false;          // measurement: host inverse iteration without the eight-at-a-time AVX-512 sweep
};

inline Switches read_switches() {
    Switches s;
    auto flag = [](const char* name) { return std::getenv(name) != nullptr; };
    s.trace = flag("NLE_TRACE");
    s.force_eig = flag("NLE_FORCE_EIG");
    s.host_solver = flag("NLE_HOST_SOLVER");
    s.host_ka = flag("NLE_HOST_KA");
    s.host_wa = flag("NLE_HOST_WA");
    s.host_q = flag("NLE_HOST_Q");
    if (const char* e = std::getenv("NLE_DEV_SOLVER_MIN")) s.dev_solver_min = std::max(3, std::atoi(e));
    if (const char* e = std::getenv("NLE_SYTRD_G")) s.sytrd_g_set = true, s.sytrd_g = std::atoi(e);
    s.nystrom_bf16x3 = flag("NLE_NYSTROM_BF16X3");
    s.no_sorted_rows = flag("NLE_NO_SORTED_ROWS");
    s.all_level_tiles = flag("NLE_ALL_LEVEL_TILES");
    s.sorted_table = flag("NLE_SORTED_TABLE");
    s.sorted_no_moments = flag("NLE_SORTED_NO_MOMENTS");
    s.gram_pairs = flag("NLE_GRAM_PAIRS");
    if (const char* e = std::getenv("NLE_SORTED_WGS_PER_CU")) s.sorted_wgs_per_cu = std::max(1, std::atoi(e));
    s.auto_stream64 = flag("NLE_AUTO_STREAM64");
    if (const char* e = std::getenv("NLE_STREAM64_CHUNK_MB")) s.stream64_chunk_mb = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("NLE_Q_SOLVER")) s.q_solver = std::strcmp(e, "lanczos") == 0 ? 1 : 0;
    s.eig_no_bisect = flag("NLE_EIG_NO_BISECT");
    s.eig_no_x8 = flag("NLE_EIG_NO_X8");
    return s;
}

}  // namespace nlesw
