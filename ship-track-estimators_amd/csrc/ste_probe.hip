// ste_probe.hip — test hooks that expose the __device__ building blocks of ste_math.h element-wise.
//
// NOT part of the ABI: the ste_probe_* names are not declared in include/ste.h and may change with the functions they
// expose.  tests/probe_binding.py binds them; tests/test_math_probe.py compares every function with a 50-digit reference
// (oracle/mp_reference.py).  A probe kernel calls the function under test and stores what it returned, nothing else, so
// what the tests see is the instruction stream the filter kernels inline.
//
// Layout: structure-of-arrays [component][count], one lane per element, lanes i >= count return.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_math.h"

namespace ste {

// ste_probe_scalar_f64 ops.  One input unless noted; out1 / flag are written only by the ops that have them.
enum ProbeScalarOp : int {
    kOpFlooredMod360 = 0,
    kOpWrap180 = 1,
    kOpRsqrtFast = 2,
    kOpDivPos = 3,  // in0 / in1
    kOpDivEarthRadius = 4,
    kOpRcpRefined = 5,
    kOpSincosKernel = 6,  // out0 = sin, out1 = cos (all sincos ops)
    kOpSincosFast = 7,
    kOpSincosDelta = 8,
    kOpAtanSmall = 9,
    kOpAtan2Fast = 10,  // atan2(in0, in1)
    kOpAsinSmall = 11,
    // N-wide forms as the kernels instantiate them: element i is slot 0, slots 1 and 2 hold fixed in-range values;
    // flag = ok (1 for the forms that have no verdict)
    kOpSincosFast3Lit = 12,
    kOpSincosFast3Reg = 13,
    kOpSincosDelta3Lit = 14,
    kOpSincosDelta3Reg = 15,
    kOpAtanSmall3Lit = 16,
    kOpAtanSmall3Reg = 17,
    kOpAsinSmall3Lit = 18,
    kOpAsinSmall3Reg = 19,
    // geodetic_finish: in0 is [8][count] = lon_r, lat_r, sp, cp, sa, ca, sd, cd; out0 = lon', out1 = lat' (degrees)
    kOpGeoFinish = 20,
    kOpGeoFinish1 = 21,
    kOpGeoFinish2 = 22,
    kOpGeoFinish3Reg = 23,
    kOpScalarCount = 24
};

enum ProbeMat4Op : int {
    kOpJacobiEig4 = 0,       // A -> V, w, out = the rotated A; status = 0x4 if the sweep cap was hit
    kOpJacobiEig4Warm = 1,   // the same, started from the given V
    kOpSymSqrt4Cold = 2,     // out = sqrt(scale * A) (clamped), V = its basis, status = sym_sqrt4's bits
    kOpSymSqrt4Warm = 3,     // the same with the given V as a valid basis
    kOpSymPinv4 = 4,         // out = pinv(A), w = eigenvalues, V = basis, status = sym_pinv4's bits
    kOpSymPinv4Block2 = 5,   // out = pinv(A) by the 2 x 2 route, w[0..1] = the block's eigenvalues (w[2..3] = 0)
    kOpLdlRightSolve4 = 6,   // out = V A^-1 (A by its upper triangle, V holds D), status = the "bad" verdict
    kOpMat4Count = 7
};

// fixed, in-range companions of the element under test in slots 1 and 2
constexpr double kFastB = 0.3, kFastC = -1.1;     // |x| < 2^20
constexpr double kDeltaB = 0.3, kDeltaC = -0.7;   // |d| <= pi/4
constexpr double kSmallB = 0.1, kSmallC = -0.3;   // |q| <= 7/16, |x| <= 1/2
// a 0.01 rad step on course 1 rad from (lon 0.1, lat 0.5): every fast path of geodetic_finish_n applies
constexpr double kGeoB[8] = {0.1, 0.5, 0.479425538604203, 0.8775825618903728, 0.8414709848078965, 0.5403023058681398,
                             0.009999833334166664, 0.9999500004166653};
constexpr double kGeoC[8] = {-0.2, -0.5, -0.479425538604203, 0.8775825618903728, -0.8414709848078965, 0.5403023058681398,
                             0.009999833334166664, 0.9999500004166653};

template <int N, class K>
__device__ __forceinline__ void probe_geo_n(const double (&g)[8], double& lon, double& lat, bool& ok) {
    double a[8][N];
    STE_UNROLL
    for (int c = 0; c < 8; ++c) {
        a[c][0] = g[c];
        if (N > 1) a[c][1 % N] = kGeoB[c];
        if (N > 2) a[c][2 % N] = kGeoC[c];
    }
    K k;
    geo_reg_init(k);
    double lon_o[N], lat_o[N];
    geodetic_finish_n<N, K>(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], lon_o, lat_o, ok, k);
    lon = lon_o[0];
    lat = lat_o[0];
}

template <int OP>
__global__ __launch_bounds__(64) void probe_scalar_kernel(size_t count, const double* in0, const double* in1, double* out0,
                                                          double* out1, int32_t* flag) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    if constexpr (OP >= kOpGeoFinish) {
        double g[8], lon, lat;
        STE_UNROLL
        for (int c = 0; c < 8; ++c) g[c] = in0[c * count + i];
        bool ok = true;
        if constexpr (OP == kOpGeoFinish) geodetic_finish(g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], lon, lat);
        if constexpr (OP == kOpGeoFinish1) probe_geo_n<1, GeoLit>(g, lon, lat, ok);
        if constexpr (OP == kOpGeoFinish2) probe_geo_n<2, GeoLit>(g, lon, lat, ok);
        if constexpr (OP == kOpGeoFinish3Reg) probe_geo_n<3, GeoReg>(g, lon, lat, ok);
        out0[i] = lon;
        out1[i] = lat;
        flag[i] = ok ? 1 : 0;
    } else if constexpr (OP >= kOpSincosFast3Lit) {
        const double a = in0[i];
        bool ok = true;
        double r0[3], r1[3];
        if constexpr (OP == kOpSincosFast3Lit || OP == kOpSincosFast3Reg) {
            using K = std::conditional_t<OP == kOpSincosFast3Reg, TrigReg, TrigLit>;
            K k;
            trig_reg_init(k);
            const double x[3] = {a, kFastB, kFastC};
            sincos_fast_n<3, K>(x, r0, r1, ok, k);
            out1[i] = r1[0];
        } else if constexpr (OP == kOpSincosDelta3Lit || OP == kOpSincosDelta3Reg) {
            using K = std::conditional_t<OP == kOpSincosDelta3Reg, TrigReg, TrigLit>;
            K k;
            trig_reg_init(k);
            const double x[3] = {a, kDeltaB, kDeltaC};
            sincos_delta_n<3, K>(x, r0, r1, ok, k);
            out1[i] = r1[0];
        } else {
            using K = std::conditional_t<OP == kOpAtanSmall3Reg || OP == kOpAsinSmall3Reg, GeoReg, GeoLit>;
            K k;
            geo_reg_init(k);
            const double x[3] = {a, kSmallB, kSmallC};
            if constexpr (OP == kOpAtanSmall3Lit || OP == kOpAtanSmall3Reg)
                atan_small_n<3, K>(x, r0, k);
            else
                asin_small_n<3, K>(x, r0, k);
        }
        out0[i] = r0[0];
        flag[i] = ok ? 1 : 0;
    } else {
        const double a = in0[i];
        double r0, r1;
        if constexpr (OP == kOpFlooredMod360) r0 = floored_mod360(a);
        if constexpr (OP == kOpWrap180) r0 = wrap180(a);
        if constexpr (OP == kOpRsqrtFast) r0 = rsqrt_fast(a);
        if constexpr (OP == kOpDivPos) r0 = div_pos(a, in1[i]);
        if constexpr (OP == kOpDivEarthRadius) r0 = div_earth_radius(a);
        if constexpr (OP == kOpRcpRefined) r0 = rcp_refined(a);
        if constexpr (OP == kOpAtanSmall) r0 = atan_small(a);
        if constexpr (OP == kOpAtan2Fast) r0 = atan2_fast(a, in1[i]);
        if constexpr (OP == kOpAsinSmall) r0 = asin_small(a);
        if constexpr (OP == kOpSincosKernel || OP == kOpSincosFast || OP == kOpSincosDelta) {
            if constexpr (OP == kOpSincosKernel) sincos_kernel(a, r0, r1);
            if constexpr (OP == kOpSincosFast) sincos_fast(a, r0, r1);
            if constexpr (OP == kOpSincosDelta) sincos_delta(a, r0, r1);
            out1[i] = r1;
        }
        out0[i] = r0;
    }
}

template <int OP>
__global__ __launch_bounds__(64) void probe_mat4_kernel(size_t count, const double* Ain, double* Vio, double* wout,
                                                        double* out, double scale, int32_t* status) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    double A[4][4], O[4][4], w[4] = {0.0, 0.0, 0.0, 0.0};
    EigBasis basis;
    double (&V)[4][4] = basis.V;
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) {
            A[r][c] = Ain[(r * 4 + c) * count + i];
            V[r][c] = Vio[(r * 4 + c) * count + i];
            O[r][c] = 0.0;
        }
    }
    int st = 0;
    if constexpr (OP == kOpJacobiEig4 || OP == kOpJacobiEig4Warm) {
        const bool ok = (OP == kOpJacobiEig4Warm) ? jacobi_eig4_warm(A, V, w) : jacobi_eig4(A, V, w);
        st = ok ? 0 : 0x4;
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            STE_UNROLL
            for (int c = 0; c < 4; ++c) O[r][c] = A[r][c];
        }
    }
    if constexpr (OP == kOpSymSqrt4Cold) {
        basis.valid = false;
        st = sym_sqrt4<false>(A, scale, O, basis);
    }
    if constexpr (OP == kOpSymSqrt4Warm) {
        basis.valid = true;
        st = sym_sqrt4<true>(A, scale, O, basis);
    }
    if constexpr (OP == kOpSymPinv4) {
        basis.valid = false;
        st = sym_pinv4<false>(A, O, basis, w);
    }
    if constexpr (OP == kOpSymPinv4Block2) {
        double w2[2];
        sym_pinv4_block2(A, O, w2);
        w[0] = w2[0];
        w[1] = w2[1];
    }
    if constexpr (OP == kOpLdlRightSolve4) {
        const double au[10] = {A[0][0], A[0][1], A[0][2], A[0][3], A[1][1], A[1][2], A[1][3], A[2][2], A[2][3], A[3][3]};
        double D[4][4];
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            STE_UNROLL
            for (int c = 0; c < 4; ++c) D[r][c] = V[r][c];
        }
        st = ldl_right_solve4(au, D, O) ? 1 : 0;
    }
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        wout[r * count + i] = w[r];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) {
            out[(r * 4 + c) * count + i] = O[r][c];
            Vio[(r * 4 + c) * count + i] = V[r][c];
        }
    }
    status[i] = st;
}

namespace {

template <int OP>
void launch_scalar(unsigned grid, hipStream_t s, size_t count, const double* in0, const double* in1, double* out0, double* out1,
                   int32_t* flag) {
    hipLaunchKernelGGL(probe_scalar_kernel<OP>, dim3(grid), dim3(64), 0, s, count, in0, in1, out0, out1, flag);
}
template <int... OPS>
void dispatch_scalar(int op, std::integer_sequence<int, OPS...>, unsigned grid, hipStream_t s, size_t count, const double* in0,
                     const double* in1, double* out0, double* out1, int32_t* flag) {
    ((op == OPS ? launch_scalar<OPS>(grid, s, count, in0, in1, out0, out1, flag) : (void)0), ...);
}
template <int OP>
void launch_mat4(unsigned grid, hipStream_t s, size_t count, const double* A, double* V, double* w, double* out, double scale,
                 int32_t* status) {
    hipLaunchKernelGGL(probe_mat4_kernel<OP>, dim3(grid), dim3(64), 0, s, count, A, V, w, out, scale, status);
}
template <int... OPS>
void dispatch_mat4(int op, std::integer_sequence<int, OPS...>, unsigned grid, hipStream_t s, size_t count, const double* A,
                   double* V, double* w, double* out, double scale, int32_t* status) {
    ((op == OPS ? launch_mat4<OPS>(grid, s, count, A, V, w, out, scale, status) : (void)0), ...);
}

}  // namespace
}  // namespace ste

extern "C" {

// in0: [count] ([8][count] for the geodetic_finish ops); in1, out0, out1: [count]; flag: [count].  Every pointer is
// required whatever the op reads or writes.
int ste_probe_scalar_f64(int32_t op, int64_t count, const double* in0, const double* in1, double* out0, double* out1,
                         int32_t* flag, void* stream) {
    if (op < 0 || op >= ste::kOpScalarCount) return ste::abi_fail(STE_EINVAL, "probe: unknown scalar op");
    if (count <= 0) return ste::abi_fail(STE_EINVAL, "probe: count must be > 0");
    if (!in0 || !in1 || !out0 || !out1 || !flag) return ste::abi_fail(STE_EINVAL, "probe: NULL pointer argument");
    const unsigned grid = (unsigned)((count + 63) / 64);
    ste::dispatch_scalar(op, std::make_integer_sequence<int, ste::kOpScalarCount>(), grid, (hipStream_t)stream, (size_t)count,
                         in0, in1, out0, out1, flag);
    return ste::abi_check_hip(hipGetLastError(), "probe_scalar launch");
}

// A: [16][count] in; V: [16][count] in / out; w: [4][count] out; out: [16][count] out; status: [count] out.
int ste_probe_mat4_f64(int32_t op, int64_t count, const double* A, double* V, double* w, double* out, double scale,
                       int32_t* status, void* stream) {
    if (op < 0 || op >= ste::kOpMat4Count) return ste::abi_fail(STE_EINVAL, "probe: unknown mat4 op");
    if (count <= 0) return ste::abi_fail(STE_EINVAL, "probe: count must be > 0");
    if (!A || !V || !w || !out || !status) return ste::abi_fail(STE_EINVAL, "probe: NULL pointer argument");
    const unsigned grid = (unsigned)((count + 63) / 64);
    ste::dispatch_mat4(op, std::make_integer_sequence<int, ste::kOpMat4Count>(), grid, (hipStream_t)stream, (size_t)count, A, V,
                       w, out, scale, status);
    return ste::abi_check_hip(hipGetLastError(), "probe_mat4 launch");
}

}  // extern "C"
