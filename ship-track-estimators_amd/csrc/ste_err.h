// ste_err.h — what the translation units of the UKF ABI share on the host: the thread-local error string behind
// ste_last_error() (one copy, in ste_kernels.hip), and the two functions of ste_forward_quad.hip that ste_kernels.hip calls.
#pragma once
#include <hip/hip_runtime.h>

namespace ste {
struct KParams;
int abi_fail(int code, const char* msg);            // records msg, returns code
int abi_check_hip(hipError_t e, const char* what);  // STE_OK or STE_ELAUNCH with the HIP error text recorded
// ste_forward_quad.hip
int choose_lanes(int B, unsigned flags);                  // lanes per track of the forward pass: 1 or 4
int launch_forward_q4(const KParams& kp, hipStream_t s);  // the quad launch of launch_forward
}  // namespace ste
