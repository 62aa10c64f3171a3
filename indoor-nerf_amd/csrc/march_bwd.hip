// Backward of the packed compositing of a grid march: nerf_march_composite's list of
// variable-length segments, differentiated with respect to raw.
//
// One wave per ray, 64 entries (a tile) per iteration, as march.hip's march_composite_kernel, whose forward
// values are formed here in the same way: delta = dist * |d|, alpha = 1 - expf(-relu(sigma) * delta),
// t = (1 - alpha) + 1e-10f, T the fp64 exclusive product of t over the ray's earlier entries (a wave scan times
// the carry of the earlier tiles), w = alpha * (float)T, the ray sums per-lane fp64 accumulators reduced once.
// The per-sample gradient arithmetic is composite.hip's composite_bwd_ray for four channels without noise,
// entropy or normals:
//   gw_j = g_rgb . c_j + g_acc' + g_weights_j + gN z_j + gA        (g_acc' = g_acc - sum g_rgb with white_bkgd,
//                                                                   depth = N / A: gN = g_depth / A, gA = -g_depth N / A^2)
//   U_j  = sum_{k > j} gw_k alpha_k prod_{j < m < k} t_m,   dL/dalpha_j = T_j (gw_j - U_j)
//   graw_j = [w_j g_rgb c_j (1 - c_j), sigma_j > 0 ? dL/dalpha_j e_j delta_j : 0]
//
// The segment is walked twice. Pass 1 is the forward's loop: it yields the sums of w and of w z, and the
// transmittance carried into tile i stays in lane i mod 64's register. Pass 2 walks the tiles from the last to the
// first: it reloads the entries, reads the tile's carry back from its lane, scans U inside the tile (common.h's
// wave_excl_suffix_affine_dpp, with the U carried in from the later tiles folded into lane 63's map) and writes
// the four gradients. A march keeps at most 4096 entries per ray, 64 tiles, so one register holds every carry.
// A longer segment is walked in super-blocks of 64 tiles from the last to the first, the carries of each refilled
// by a forward walk from the segment's start up to the super-block's end: quadratic in the number of super-blocks,
// correct for any length, never taken by a real march. No LDS, no atomics: identical inputs give identical bits.
#include "common.h"

namespace nerf {

constexpr int kPackedBwdThreads = 256;
constexpr int kPackedBwdWaves = kPackedBwdThreads / 64;   // rays per block, as march.hip's kMarchWaves

struct PackedCompositeBwdArgs {
    const float* raw;        // [n, 4]
    const float* z;          // [n]
    const float* dist;       // [n]
    const int32_t* off;      // [R + 1]
    const float* rays_d;     // [R, 3]
    int64_t R, n;
    int white;
    const float* g_rgb;      // optional [R, 3]
    const float* g_disp;     // optional [R]
    const float* g_acc;      // optional [R]
    const float* g_depth;    // optional [R]
    const float* g_w;        // optional [n]
    float* graw;             // out [n, 4]
};

// composite_common.h's sigmoidf
__device__ __forceinline__ float packed_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// alpha and t of entry j of the list (a lane past the segment's end: alpha 0, t 1, which changes no product)
__device__ __forceinline__ void packed_alpha(const PackedCompositeBwdArgs& a, int64_t j, int64_t end, float norm_d,
                                             float& sg, float& delta, float& e, float& alpha, float& t) {
    sg = 0.f; delta = 0.f; e = 1.f; alpha = 0.f; t = 1.f;
    if (j < end) {
        delta = a.dist[j] * norm_d;
        sg = a.raw[4 * j + 3];
        const float relu_s = sg > 0.f ? sg : 0.f;
        e = expf(-relu_s * delta);
        alpha = 1.0f - e;
        t = (1.0f - alpha) + 1e-10f;
    }
}

__global__ void __launch_bounds__(kPackedBwdThreads) packed_composite_bwd_kernel(PackedCompositeBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kPackedBwdWaves + (threadIdx.x >> 6);
    if (r >= a.R) return;   // wave-uniform: every lane of a live wave takes part in the scans below
    const float dx = a.rays_d[3 * r], dy = a.rays_d[3 * r + 1], dz = a.rays_d[3 * r + 2];
    const float norm_d = sqrtf(dx * dx + dy * dy + dz * dz);
    // the segment, held inside the list whatever the offsets say (march_composite_kernel's clamp)
    int64_t end = a.off[r + 1], beg = a.off[r];
    end = end < 0 ? 0 : (end > a.n ? a.n : end);
    beg = beg < 0 ? 0 : (beg > end ? end : beg);
    if (beg >= end) return;   // wave-uniform: an empty segment writes nothing
    const int64_t n_tiles = (end - beg + 63) / 64;
    const int64_t n_super = (n_tiles + 63) / 64;

    // per-ray upstream gradients (composite_bwd_ray's); gN and gA once the sums are known
    float gr0 = 0.f, gr1 = 0.f, gr2 = 0.f;
    if (a.g_rgb) { gr0 = a.g_rgb[3 * r]; gr1 = a.g_rgb[3 * r + 1]; gr2 = a.g_rgb[3 * r + 2]; }
    float g_acc = a.g_acc ? a.g_acc[r] : 0.f;
    if (a.white) g_acc = g_acc - ((gr0 + gr1) + gr2);     // rgb_map + (1 - acc)
    float gN = 0.f, gA = 0.f;
    bool use_depth = false;

    double U_in = 0.0;   // U at the last entry of the tile in hand: the later tiles' maps applied to 0
    for (int64_t sb = n_super - 1; sb >= 0; --sb) {
        const int64_t t_lo = sb * 64, t_hi = n_tiles < t_lo + 64 ? n_tiles : t_lo + 64;
        const bool sums = sb == n_super - 1;   // the first walk covers the whole segment: the ray sums
        // ---- pass 1: the forward over tiles [0, t_hi); the carry into tile t_lo + i stays in lane i
        double carry = 1.0, carries = 1.0, acc = 0, dn = 0;
        for (int64_t ti = 0; ti < t_hi; ++ti) {
            if (ti >= t_lo && lane == (int)(ti - t_lo)) carries = carry;
            const int64_t j = beg + ti * 64 + lane;
            float sg, delta, e, alpha, t;
            packed_alpha(a, j, end, norm_d, sg, delta, e, alpha, t);
            const double excl = wave_excl_prod_dpp((double)t);
            if (sums) {
                const double T = carry * excl;
                const float w = alpha * (float)T;
                const float zj = j < end ? a.z[j] : 0.f;
                acc += (double)w;
                dn += (double)(w * zj);
            }
            carry = carry * readlane_d(excl * (double)t, 63);
        }
        if (sums) {
            const float facc = (float)wave_sum_dpp(acc);
            const float num = (float)wave_sum_dpp(dn);
            const float depth = num / facc;   // NaN at 0 / 0, as the forward
            float g_depth = a.g_depth ? a.g_depth[r] : 0.f;
            if (a.g_disp) {   // disp = 1 / fmaxf(1e-10, depth)
                const float gd = a.g_disp[r];
                if (gd != 0.f) {
                    const float m = fmaxf(1e-10f, depth);
                    const float gm = -gd / (m * m);
                    if (depth > 1e-10f || depth != depth) g_depth += gm;
                    else if (depth == 1e-10f) g_depth += 0.5f * gm;
                }
            }
            use_depth = g_depth != 0.f;
            if (use_depth) {
                gN = g_depth / facc;
                gA = -g_depth * num / (facc * facc);
            }
        }
        // ---- pass 2: tiles t_hi - 1 down to t_lo
        for (int64_t ti = t_hi - 1; ti >= t_lo; --ti) {
            const int src = __builtin_amdgcn_readfirstlane((int)(ti - t_lo));
            const double Tc = readlane_d(carries, src);
            const int64_t j = beg + ti * 64 + lane;
            float sg, delta, e, alpha, t;
            packed_alpha(a, j, end, norm_d, sg, delta, e, alpha, t);
            const double T = Tc * wave_excl_prod_dpp((double)t);
            const float w = alpha * (float)T;
            float c0 = 0.f, c1 = 0.f, c2 = 0.f, gw = 0.f;
            if (j < end) {
                c0 = packed_sigmoid(a.raw[4 * j]); c1 = packed_sigmoid(a.raw[4 * j + 1]);
                c2 = packed_sigmoid(a.raw[4 * j + 2]);
                gw = (gr0 * c0 + gr1 * c1) + gr2 * c2;
                gw += g_acc;
                if (a.g_w) gw += a.g_w[j];
                if (use_depth) gw += gN * a.z[j] + gA;
            }
            // U_{j-1} = gw_j alpha_j + t_j U_j: the tile's maps, lane 63's applied to the U carried in
            const double X = (double)gw * (double)alpha;
            const double P = (double)t;
            double U = wave_excl_suffix_affine_dpp(lane == 63 ? X + P * U_in : X, P, lane);
            if (lane == 63) U = U_in;
            const double galpha = T * ((double)gw - U);
            U_in = readlane_d(X + P * U, 0);   // U at the last entry of the tile before
            if (j < end) {
                float* g = a.graw + 4 * j;
                g[0] = (w * gr0) * (c0 * (1.0f - c0));
                g[1] = (w * gr1) * (c1 * (1.0f - c1));
                g[2] = (w * gr2) * (c2 * (1.0f - c2));
                g[3] = sg > 0.f ? (float)galpha * e * delta : 0.f;
            }
        }
    }
}

}  // namespace nerf

using namespace nerf;

extern "C" int nerf_packed_composite_bwd(const float* d_raw, const float* d_z, const float* d_dist,
                                         const int32_t* d_offsets, const float* d_rays_d, int64_t n_rays,
                                         int64_t n_points, int white_bkgd, const float* d_g_rgb,
                                         const float* d_g_disp, const float* d_g_acc, const float* d_g_depth,
                                         const float* d_g_weights, float* d_graw, void* stream) {
    NERF_REQUIRE(n_rays >= 0 && n_rays <= INT32_MAX, "packed_composite_bwd: n_rays %lld", (long long)n_rays);
    NERF_REQUIRE(n_points >= 0 && n_points <= INT32_MAX, "packed_composite_bwd: n_points %lld", (long long)n_points);
    if (n_rays == 0 || n_points == 0) return NERF_OK;   // every segment is empty: nothing is written
    NERF_REQUIRE(d_raw && d_z && d_dist && d_offsets && d_rays_d && d_graw, "packed_composite_bwd: null arg");
    PackedCompositeBwdArgs a{};
    a.raw = d_raw; a.z = d_z; a.dist = d_dist; a.off = d_offsets; a.rays_d = d_rays_d; a.R = n_rays; a.n = n_points;
    a.white = white_bkgd ? 1 : 0; a.g_rgb = d_g_rgb; a.g_disp = d_g_disp; a.g_acc = d_g_acc; a.g_depth = d_g_depth;
    a.g_w = d_g_weights; a.graw = d_graw;
    hipLaunchKernelGGL(packed_composite_bwd_kernel, dim3(blocks_for(n_rays, kPackedBwdWaves)),
                       dim3(kPackedBwdThreads), 0, as_stream(stream), a);
    NERF_CHECK_LAUNCH("packed_composite_bwd");
    return NERF_OK;
}
