// Early ray termination for forward-only rendering.
//
// A field call over pts [R, S, 3] runs front to back in slabs [s0, s1) of samples. Every ray is alive in
// slab 0; after the field has run on a slab that is not the last, each ray still alive advances its
// optical depth over that slab's samples (ert_advance_kernel) and dies for every later slab once
// tau > tau_max = -log(eps): its transmittance is below eps, so nothing behind that point can change
// the pixel by more than eps.
//
// The rule (one thread per ray, fp32, strictly in sample order; the file is built with -ffp-contract=off,
// so no multiply-add is fused): norm_d = sqrtf(dx*dx + dy*dy + dz*dz) as composite_common.h's
// ray_forward; for i in [s0, s1): d = (z[i+1] - z[i]) * norm_d, s = sigma_i > 0 ? sigma_i : 0 (NaN gives
// 0), tau = tau + s * d. s1 < S always (no decision follows the last slab), so z[i+1] exists and
// compositing's 1e10 last delta is never needed. The same bits as its NumPy fp32 restatement
// (tests/test_gpu_early_stop.py).
//
// The compaction of one slab's kept samples (nerf_ert_compact) is sparse_points.hip: a sample of a dead ray
// is not kept and gets an all-zero raw row, so the result is the dense render with sigma masked per sample.
#include "common.h"

namespace nerf {

// one thread per ray: R x (s1 - s0) strided sigma reads, small against the field call of the slab
__global__ void __launch_bounds__(256) ert_advance_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                          const float* __restrict__ rays_d, int64_t R, int S, int s0,
                                                          int s1, float tau_max, float* __restrict__ tau,
                                                          uint8_t* __restrict__ alive, int32_t* __restrict__ stop) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R || !alive[r]) return;
    const float dx = rays_d[3 * r + 0], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
    const float norm_d = sqrtf(dx * dx + dy * dy + dz * dz);
    const float* zr = z + r * S;
    const float* rr = raw + 4 * (r * S) + 3;
    float t = tau[r];
    for (int i = s0; i < s1; ++i) {      // s1 < S: zr[i + 1] exists
        const float d = (zr[i + 1] - zr[i]) * norm_d;
        const float sg = rr[4 * i];
        const float s = sg > 0.f ? sg : 0.f;
        t = t + s * d;
    }
    tau[r] = t;
    if (t > tau_max) {
        alive[r] = 0;
        stop[r] = s1;
    }
}

}  // namespace nerf

using namespace nerf;

extern "C" int nerf_ert_advance(const float* d_raw, const float* d_z, const float* d_rays_d, int64_t n_rays,
                                int64_t samples_per_ray, int64_t s0, int64_t s1, float tau_max, float* d_tau,
                                uint8_t* d_alive, int32_t* d_stop, void* stream) {
    NERF_REQUIRE(samples_per_ray >= 1 && samples_per_ray <= INT32_MAX, "ert_advance: samples_per_ray %lld",
                 (long long)samples_per_ray);
    NERF_REQUIRE(n_rays >= 0 && n_rays <= INT32_MAX / samples_per_ray, "ert_advance: n_rays %lld x %lld samples",
                 (long long)n_rays, (long long)samples_per_ray);
    // s1 < S: the rule is applied after a slab that is not the last, and reads z[s1]
    NERF_REQUIRE(s0 >= 0 && s0 <= s1 && s1 < samples_per_ray,
                 "ert_advance: slab [%lld, %lld) must end before the last of %lld samples", (long long)s0,
                 (long long)s1, (long long)samples_per_ray);
    NERF_REQUIRE(tau_max > 0.f, "ert_advance: tau_max %g must be positive", (double)tau_max);
    if (n_rays == 0) return NERF_OK;
    NERF_REQUIRE(d_raw && d_z && d_rays_d && d_tau && d_alive && d_stop, "ert_advance: null arg");
    hipLaunchKernelGGL(ert_advance_kernel, dim3(blocks_for(n_rays, 256)), dim3(256), 0, as_stream(stream), d_raw, d_z,
                       d_rays_d, n_rays, (int)samples_per_ray, (int)s0, (int)s1, tau_max, d_tau, d_alive, d_stop);
    NERF_CHECK_LAUNCH("ert_advance");
    return NERF_OK;
}
