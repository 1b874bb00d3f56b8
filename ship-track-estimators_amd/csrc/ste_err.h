// ste_err.h — what the translation units of the UKF ABI share on the host: the thread-local error string behind
// ste_last_error() (one copy, in ste_kernels.hip), with_bool (a run-time flag as a template argument of a launch), and the
// functions of ste_forward_quad.hip, ste_smooth.hip, ste_sample.hip and ste_lagone.hip that ste_kernels.hip calls, and the
// refusals and the row length that the entries downstream of the smoother share (Refusal, track_ld).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <type_traits>

#include "../../include/ste.h"

namespace ste {
struct KParams;
struct NoiseParams;
struct SmoothSchedParams;
int abi_fail(int code, const char* msg);            // records msg, returns code
int abi_check_hip(hipError_t e, const char* what);  // STE_OK or STE_ELAUNCH with the HIP error text recorded
// ste_forward_quad.hip
int choose_lanes(int B, unsigned flags);                  // lanes per track of the forward pass: 1 or 4
int launch_forward_q4(const KParams& kp, hipStream_t s);  // the quad launch of launch_forward
// ste_smooth.hip
bool lean_smoother(const KParams& kp);  // does the batch smooth with the two-kernel form?
int launch_backward_work(const KParams& kp, const NoiseParams* np, hipStream_t s);  // launch_backward with rts_work
int launch_recur_sched(bool shift, bool plain, int nitems, const SmoothSchedParams& sp, hipStream_t s);  // plain: every window is
// ste_sample.hip
int launch_sample_coef(const KParams& kp, const ste_ukf_noise_f64* nz, const ste_ukf_sample_f64& sm, hipStream_t s);
int launch_sample_recur(const KParams& kp, const ste_ukf_sample_f64& sm, hipStream_t s);
// ste_lagone.hip
int launch_lag_one(const KParams& kp, const ste_ukf_noise_f64* nz, const ste_lag_one_f64& lg, hipStream_t s);

// The refusals of one extern "C" entry: holds the call's name once; refuse(why) records "<call>: <why>" and returns
// STE_EINVAL.  The checks that every entry downstream of the smoother opens with return STE_OK, or refuse with the fixed phrase
// of include/ste.h.  Nothing is built on the way to STE_OK: the text is put together only when refusing.
struct Refusal {
    const char* call;
    int operator()(const std::string& why) const { return abi_fail(STE_EINVAL, (std::string(call) + ": " + why).c_str()); }
    int shape(const ste_ukf_batch_f64* b) const {
        return b->B <= 0 || b->Nmax < 0 ? (*this)("B must be > 0 and Nmax >= 0") : STE_OK;
    }
    int stride(const ste_ukf_batch_f64* b) const {
        return b->track_stride != 0 && b->track_stride < b->B
                   ? (*this)("track_stride must be 0 or >= B (a window inside rows of track_stride tracks)")
                   : STE_OK;
    }
    // arg: the argument as the caller knows it ("pm->nstates"); note: what limits it, " (...)" or nothing
    int nstates(const char* arg, int n, const char* note = "") const {
        if (n < 1) return (*this)(std::string(arg) + " must be >= 1");
        if (n > 65535) return (*this)(std::string(arg) + " is limited to 65535 per call" + note);
        return STE_OK;
    }
    // when: " when <output> is asked for" where only that output needs a model, or nothing
    int model(const char* arg, int m, const char* when = "") const {
        return m != STE_PREP_SPHERE && m != STE_PREP_WGS84
                   ? (*this)(std::string(arg) + " must be STE_PREP_SPHERE or STE_PREP_WGS84" + when)
                   : STE_OK;
    }
};

// tracks per row of the batch's arrays: track_stride, or B
inline size_t track_ld(const ste_ukf_batch_f64* b) { return (size_t)(b->track_stride ? b->track_stride : b->B); }

// A run-time flag as a compile-time constant: f(std::true_type{}) or f(std::false_type{})
template <class F>
auto with_bool(bool v, F&& f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}
}  // namespace ste
