// ste_err.h — what the translation units of the UKF ABI share on the host: the thread-local error string behind
// ste_last_error() (one copy, in ste_kernels.hip), with_bool (a run-time flag as a template argument of a launch), and the
// functions of ste_forward_quad.hip, ste_smooth.hip, ste_sample.hip and ste_lagone.hip that ste_kernels.hip calls.
#pragma once
#include <hip/hip_runtime.h>

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
int launch_recur_sched(bool shift, int nitems, const SmoothSchedParams& sp, hipStream_t s);
// ste_sample.hip
int launch_sample_coef(const KParams& kp, const ste_ukf_noise_f64* nz, const ste_ukf_sample_f64& sm, hipStream_t s);
int launch_sample_recur(const KParams& kp, const ste_ukf_sample_f64& sm, hipStream_t s);
// ste_lagone.hip
int launch_lag_one(const KParams& kp, const ste_ukf_noise_f64* nz, const ste_lag_one_f64& lg, hipStream_t s);

// A run-time flag as a compile-time constant: f(std::true_type{}) or f(std::false_type{})
template <class F>
auto with_bool(bool v, F&& f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}
}  // namespace ste
