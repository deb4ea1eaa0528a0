// nufft_device.h -- the interpolation kernel of the trajectory operator and its window arithmetic, shared by nufft_kernels.hip and dcf_kernels.hip
// (DESIGN.md sections 14 and 21): both evaluate psi with this one function on the same inputs.
#pragma once

namespace nudev {

__device__ __forceinline__ double nu_phi(double d, double inv_hw, double beta) {
    const double z = d * inv_hw, t = 1.0 - z * z;
    return t >= 0.0 ? exp(beta * (sqrt(t) - 1.0)) : 0.0;
}
__device__ __forceinline__ int nu_k0(double u, double hw) { return (int)ceil(u - hw); }    // first grid point of the window [k0, k0 + w)
__device__ __forceinline__ int nu_wrap(int k, int G) { k %= G; return k < 0 ? k + G : k; }

}  // namespace nudev
