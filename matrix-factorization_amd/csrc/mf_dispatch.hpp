// mf_dispatch.hpp -- runtime (dtype, n_factors, kernel) -> template dispatch.
#pragma once

#include "mf_common.hpp"

namespace mf {

// ------------------------------------------------------------ dispatch
// What dispatch() can serve, refused in entry point fn's name.  An entry point
// that returns early for empty input calls this first, so that bad codes are
// refused whatever the sizes.
inline int check_model(const char* fn, int dtype, int k, int kernel) {
    if (dtype != MF_F32 && dtype != MF_F64)
        set_error("%s: dtype=%d (must be MF_F32 or MF_F64)", fn, dtype);
    else if (kernel < MF_LINEAR || kernel > MF_RBF)
        set_error("%s: kernel=%d (must be MF_LINEAR, MF_SIGMOID or MF_RBF)", fn, kernel);
    else if (k < 0 || k > kMaxFactors)
        set_error("%s: n_factors=%d (must be in [0, %d])", fn, k, kMaxFactors);
    else
        return MF_OK;
    return MF_ERR_INVALID;
}

// Calls F.template run<T, GS, V, KERN>() for the runtime (dtype, k, kernel).
template <typename F>
inline int dispatch(const char* fn, int dtype, int k, int kernel, F&& f) {
    if (check_model(fn, dtype, k, kernel) != MF_OK) return MF_ERR_INVALID;
    const int kp = kpad_of(k);
#define MF_KCASE(T, KP, GS, V)                                                   \
    if (kp == KP) {                                                              \
        if (kernel == MF_LINEAR) return f.template run<T, GS, V, MF_LINEAR>();   \
        if (kernel == MF_SIGMOID) return f.template run<T, GS, V, MF_SIGMOID>(); \
        return f.template run<T, GS, V, MF_RBF>();                               \
    }
#define MF_TCASES(T)                \
    MF_KCASE(T, 16, 16, 1)          \
    MF_KCASE(T, 32, 32, 1)          \
    MF_KCASE(T, 64, 64, 1)          \
    MF_KCASE(T, 128, 64, 2)         \
    MF_KCASE(T, 256, 64, 4)         \
    MF_KCASE(T, 512, 64, 8)         \
    MF_KCASE(T, 1024, 64, 16)
    if (dtype == MF_F32) { MF_TCASES(float) }
    else { MF_TCASES(double) }
#undef MF_TCASES
#undef MF_KCASE
    set_error("internal: no kernel for n_factors=%d", k);
    return MF_ERR_INVALID;
}

}  // namespace mf
