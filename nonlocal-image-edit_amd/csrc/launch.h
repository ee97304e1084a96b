// Host side of every kernel that is instantiated per size or launched with dynamic LDS: the map from the run-time count
// onto its instantiation and the launch itself.  Not installed, not part of kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

namespace nlek {

// f(std::integral_constant<int, V>{}) for the listed V that equals v; false (and no call) where v is none of them.
// The rules on which forms a value has are written in f, as `if constexpr` on V; two run-time values nest two dispatches.
template <int... V, class F>
bool dispatch_values(int v, F&& f) {
    return ((v == V ? (f(std::integral_constant<int, V>{}), true) : false) || ...);
}
// the contiguous case: every NC in [LO, HI]
template <int LO, class F, int... I>
bool dispatch_columns_seq(int nc, F&& f, std::integer_sequence<int, I...>) {
    return dispatch_values<(LO + I)...>(nc, f);
}
template <int LO, int HI, class F>
bool dispatch_columns(int nc, F&& f) {
    return dispatch_columns_seq<LO>(nc, f, std::make_integer_sequence<int, HI - LO + 1>{});
}

// Launches `kernel`; beyond 48 KB of dynamic LDS the limit of exactly this instantiation is raised first.
template <class... P, class... A>
hipError_t launch(void (*kernel)(P...), dim3 grid, dim3 threads, size_t shm, hipStream_t s, A&&... args) {
    if (shm > 48 * 1024) {
        hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        if (ea != hipSuccess) return ea;
    }
    hipLaunchKernelGGL(kernel, grid, threads, shm, s, static_cast<P>(args)...);
    return hipGetLastError();
}

}  // namespace nlek
