// Host-side launch helpers: run-time values to template arguments, and the attribute a kernel needs for more than 64 KB of dynamic LDS.
//
//   cfd_dispatch([&](auto V, auto NJ, auto T) { hipLaunchKernelGGL((k<CFD_B(V), CFD_I(NJ), CFD_T(T)>), ...); },
//                vec, cfd_among<1, 2, 3, 4, 5>(nj), cfd_storage(dt));
//
// Each choice reaches the generic lambda as a type that carries a compile-time constant, one instantiation of the lambda per combination.
// A combination that must not exist is pruned by `if constexpr` on those constants inside the lambda.
#pragma once
#include <atomic>
#include <mutex>
#include <type_traits>

#include "cfd_common.h"

#define CFD_B(c) decltype(c)::value           // a bool choice
#define CFD_I(c) decltype(c)::value           // a cfd_among choice
#define CFD_T(c) typename decltype(c)::type   // a cfd_storage choice

// an int that is one of Vs; any other value takes the LAST of them (the `default:` of the switch this replaces)
template <int... Vs>
struct cfd_among_t { int v; };
template <int... Vs>
static inline cfd_among_t<Vs...> cfd_among(int v) { return {v}; }
// activation storage: CFD_DT_BF16 -> __bf16, anything else -> float
struct cfd_storage { int dt; explicit cfd_storage(int dt_) : dt(dt_) {} };
template <typename T>
struct cfd_type { using type = T; };

template <typename F>
static void cfd_dispatch(F&& f) { f(); }
template <typename F, typename... Rest>
static void cfd_dispatch(F&& f, bool b, Rest... rest);
template <typename F, typename... Rest>
static void cfd_dispatch(F&& f, cfd_storage s, Rest... rest);
template <typename F, int V0, int... Vs, typename... Rest>
static void cfd_dispatch(F&& f, cfd_among_t<V0, Vs...> c, Rest... rest);

// f(C{}, <the constants of rest>...)
template <typename C, typename F, typename... Rest>
static void cfd_dispatch_bind(F&& f, Rest... rest) {
    cfd_dispatch([&](auto... c) { f(C{}, c...); }, rest...);
}
template <typename F, typename... Rest>
static void cfd_dispatch(F&& f, bool b, Rest... rest) {
    if (b) cfd_dispatch_bind<std::true_type>(f, rest...);
    else cfd_dispatch_bind<std::false_type>(f, rest...);
}
template <typename F, typename... Rest>
static void cfd_dispatch(F&& f, cfd_storage s, Rest... rest) {
    if (s.dt == CFD_DT_BF16) cfd_dispatch_bind<cfd_type<__bf16>>(f, rest...);
    else cfd_dispatch_bind<cfd_type<float>>(f, rest...);
}
template <typename F, int V0, int... Vs, typename... Rest>
static void cfd_dispatch(F&& f, cfd_among_t<V0, Vs...> c, Rest... rest) {
    if constexpr (sizeof...(Vs) == 0) {
        cfd_dispatch_bind<std::integral_constant<int, V0>>(f, rest...);
    } else {
        if (c.v == V0) cfd_dispatch_bind<std::integral_constant<int, V0>>(f, rest...);
        else cfd_dispatch(f, cfd_among_t<Vs...>{c.v}, rest...);
    }
}
// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): the all-flags case under its first name
template <typename F, typename... Bools>
static void with_bools(F&& f, Bools... b) { cfd_dispatch(f, static_cast<bool>(b)...); }

// A kernel that is launched with more than 64 KB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize first.  The attribute
// belongs to the (kernel, device) pair: it is set once per pair (again only for a larger size), what is set is published per device, the
// slow path runs under a lock, and a failure is the caller's error.  `bytes`: what this launch asks for, or the most the kernel is ever
// launched with; up to 64 KB nothing is needed.  (Internal linkage: one table per kernel instantiation, nothing exported.)
#define CFD_LDS_MAX_DEVICES 64
template <auto Kernel>
static int cfd_allow_lds(size_t bytes, const char* fn) {
    if (bytes <= 64 * 1024) return CFD_OK;
    static std::atomic<size_t> allowed[CFD_LDS_MAX_DEVICES];  // (zero-initialised)
    static std::mutex mu;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    CFD_REQUIRE(e == hipSuccess && dev >= 0 && dev < CFD_LDS_MAX_DEVICES, CFD_ERR_HIP, "%s: no current device (%s, device %d)", fn,
                hipGetErrorString(e), dev);
    if (allowed[dev].load(std::memory_order_acquire) >= bytes) return CFD_OK;
    std::lock_guard<std::mutex> lock(mu);
    if (allowed[dev].load(std::memory_order_relaxed) >= bytes) return CFD_OK;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    CFD_REQUIRE(e == hipSuccess, CFD_ERR_HIP, "%s: %zu bytes of dynamic LDS refused: %s", fn, bytes, hipGetErrorString(e));
    allowed[dev].store(bytes, std::memory_order_release);
    return CFD_OK;
}
