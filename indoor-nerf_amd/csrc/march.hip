// Grid ray marching for forward-only rendering: a ray's samples in occupied cells as a packed
// variable-length list, and the compositing of such a list. The dense [R, K] arrays are never formed.
//
// The lattice of a packed ray row [o, d, near, far(, viewdir)] with the sampler's table t [K] (every operation
// fp32 and written out; the file is built with -ffp-contract=off, so these are the bits of sampling.hip's
// unperturbed coarse samples with lindisp = 0):
//   z_k = near * (1.0f - t_k) + far * t_k;   p_k = o + d * z_k per axis;
//   dist_k = z_{k+1} - z_k for k < K - 1, 1e10f for k = K - 1: the distance to the next LATTICE sample, kept
//   or not, which is what compositing computes from the dense z.
// Sample k of ray r is kept when p_k is inside the box and its cell's bit is set (occ_common.h's cell rule, the
// answer of nerf_occ_query). The kept samples of ray r, in ascending k, are entries [off[r], off[r + 1]) of
// the list, rays ascending: the list is the dense array's kept entries in row-major order.
//
// One wave per ray, lane l of iteration i tests lattice index 64 i + l; a ballot counts the kept lanes.
//   nerf_march_count: counts [R] (one store per ray); then, per block of kCompactBlock rays, the sum of its counts
//     (a reduction of its own: one atomic add per ray into the few counters of a chunk, all in one cache line,
//     took longer than the walk itself); then off [R + 1], the exclusive scan of counts, by
//     compact_common.h's block offsets and a scan inside each block.
//   nerf_march_write: the same walk; a kept sample's rank is off[r] + the kept samples of the ray's earlier
//     iterations + the kept lanes below its own. Writes pts_c, z_c, dist_c and the ray's SH4 row per point.
//   nerf_march_composite: packed forward compositing, one wave per ray, 64 entries per iteration. The
//     per-sample arithmetic is composite_common.h's ray_forward restated (that header is on the training path
//     and is not touched from here): sigmoid, relu, expf(-relu_s * dist * |d|), alpha = 1 - e,
//     t = (1 - alpha) + 1e-10f, w = alpha * (float)T with T the fp64 exclusive product of t over the ray's
//     earlier entries (a wave scan times a running carry); the ray sums are per-lane fp64 accumulators,
//     reduced once. A skipped sample has alpha = 0 and t = 1.0f exactly, so leaving it out changes no
//     product and no sum as a real number; only the fp64 association differs from the dense kernel.
//
// Stopping opaque rays inside the march: the K lattice indices run front to back in slabs
// [k0, k1); a ray is walked only while its flag alive[r] is set.
//   nerf_slab_march_count / nerf_slab_march_write: the two walks above over the lattice range [k0, k1) of the rays
//     with alive[r] != 0 (NULL: every ray); a dead ray counts 0. dist_k still comes from the full lattice (1e10f
//     for k = K - 1 only). nerf_march_count / nerf_march_write are these with 0, K, NULL.
//   nerf_slab_march_composite: march_composite_kernel with a per-ray fp64 state [R, 6] (the carry, the three sums
//     of w c, of w and of w z) read at entry unless `first` and written at exit unless `last`; the maps are
//     written on `last`. first = last = 1 is nerf_march_composite bit for bit; over several slabs only the fp64
//     association differs (each slab's lane sums are reduced before the next slab adds to them).
//   nerf_slab_march_advance: the stopping rule, one thread per ray, fp32, strictly in entry order (the file is
//     built with -ffp-contract=off): norm_d = sqrtf(dx*dx + dy*dy + dz*dz); for each entry e of the ray's segment:
//     d = dist[e] * norm_d, s = sigma_e > 0 ? sigma_e : 0 (NaN gives 0), tau = tau + s * d; the ray dies
//     (alive = 0, stop = s1) when tau > tau_max. early_stop.hip's rule with the packed dist in place of
//     z[i + 1] - z[i]; a skipped lattice sample adds nothing, as a masked sigma does there.
//
// SH through a ray index: the view encoding is the same for every sample of a ray, so the list can
// carry the ray's row number (4 B per point) instead of its SH4 row (64 B per point).
//   nerf_ray_sh_records: one thread per packed ray row; the kShRecord record of the row's view direction (columns
//     8..10): sh4_eval, 16 fp32 coefficients, then the three bf16 pieces of each. sampling.hip's
//     sample_stratified_kernel writes the same record per ray; its lines are restated here (that file is on the
//     training path and is not touched), and both files are built with -ffp-contract=off, so the bits agree.
//   nerf_rays_march_write / nerf_rays_slab_march_write: march_write_kernel<true>: the write's walk with
//     ray_c[idx] = r in place of the SH row; no SH is evaluated and rows of 8 columns are accepted.
//
// A jittered lattice: nerf_jitter_march_count / nerf_jitter_march_write walk the whole lattice with
// sample k of ray r at the depth sampling.hip's sample_stratified_kernel writes with lindisp = 0, perturb = 1 (its
// lines restated in jitter_depth; that file is on the training path and is not touched; both files are built with
// -ffp-contract=off, so the bits agree). With b_k = march_depth(t_k):
//   lower = k > 0 ? 0.5f * (b_k + b_{k-1}) : b_k;   upper = k + 1 < K ? 0.5f * (b_{k+1} + b_k) : b_k;
//   z_k = lower + (upper - lower) * u,   u = d_u[r K + k], else philox_uniform(seed, offset, r K + k) with the pair
//   from d_rng if given, else the host's (the sampler's precedence);
//   p_k = o + d * z_k, kept by the cell rule; dist_k = z_{k+1} - z_k of the JITTERED depths, 1e10f for k = K - 1.
// These are kernels of their own (jitter_count_kernel, jitter_write_kernel<kRays>) with the jitter's arguments in a
// second kernel parameter: march_sample, the plain kernels and MarchArgs' layout are as they were, so the unjittered
// entries keep their code and their bits.
//   Philox: one philox_uniform per lane and iteration, three of its four outputs unused. A wave pays for a VALU
//     instruction whether 16 or 64 of its lanes are active, so 16 lanes evaluating philox_uniform4 for the 64 samples
//     of ONE iteration would issue the same ten rounds and add four cross-lane moves; sharing pays only if one
//     evaluation serves four iterations (256 samples), which needs the K % 4 != 0 straddle handled per ray (the
//     groups of four are groups of r K + k, not of k) and a staging buffer. Per lane and iteration the index r K + k
//     goes straight into philox_uniform, so a group that straddles two rays is simply evaluated by the lanes of both
//     rays' waves: the bits are philox_uniform(..., r K + k) by construction.
//   The next sample's depth: the write walks one iteration ahead. Iteration i + 1's depths (its Philox, its cell
//     tests) are computed before iteration i is stored; lane l < 63 takes z_{k+1} from lane l + 1 (__shfl_down) and
//     lane 63 from lane 0 of the iteration ahead (a broadcast of that lane, __shfl). Every depth is evaluated exactly once: K per ray and
//     no 65th per iteration. The count walk needs z_k only.
#include "compact_common.h"
#include "occ_common.h"

namespace nerf {

constexpr int kMarchThreads = 256;
constexpr int kMarchWaves = kMarchThreads / 64;   // rays per block
constexpr int kMarchMaxSamples = 4096;

struct MarchArgs {
    OccGrid g;
    const uint32_t* bits;
    const float* rays;       // [R, C]
    int64_t R;
    int C, K;
    int k0, k1;              // the lattice range walked, 0 <= k0 <= k1 <= K
    const uint8_t* alive;    // optional [R]: a ray with alive[r] == 0 keeps nothing
    const float* t;          // [K]
    int32_t* counts;         // [R]
    int32_t* off;            // [R + 1]
    float* rays_d;           // optional out [R, 3]
    int32_t* block_counts;   // workspace [ceil(R / kCompactBlock)]
    int64_t capacity;        // rows of the packed outputs
    float* pts_c;            // out [capacity, 3]
    float* z_c;              // out [capacity]
    float* dist_c;           // out [capacity]
    float* sh_c;             // optional out [capacity, 16] (C == 11)
    int32_t* ray_c;          // march_write_kernel<true>: out [capacity], the row number of the entry's ray
};

struct MarchRay {
    float o[3], d[3], near, far;
};

__device__ __forceinline__ MarchRay march_ray(const MarchArgs& a, int64_t r) {
    const float* ray = a.rays + r * a.C;
    MarchRay m;
    m.o[0] = ray[0]; m.o[1] = ray[1]; m.o[2] = ray[2];
    m.d[0] = ray[3]; m.d[1] = ray[4]; m.d[2] = ray[5];
    m.near = ray[6]; m.far = ray[7];
    return m;
}

// sampling.hip's base_depth with lindisp = 0
__device__ __forceinline__ float march_depth(const MarchRay& m, float t) { return m.near * (1.0f - t) + m.far * t; }

// lattice sample k < K of the ray: its depth, its position and whether it is kept
__device__ __forceinline__ bool march_sample(const MarchArgs& a, const MarchRay& m, int k, float& z, float* p) {
    z = march_depth(m, a.t[k]);
    p[0] = m.o[0] + m.d[0] * z;
    p[1] = m.o[1] + m.d[1] * z;
    p[2] = m.o[2] + m.d[2] * z;
    return occ_occupied(a.g, a.bits, p);
}

__global__ void __launch_bounds__(kMarchThreads) march_count_kernel(MarchArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kMarchWaves + (threadIdx.x >> 6);
    if (r >= a.R) return;   // wave-uniform
    const MarchRay m = march_ray(a, r);
    const int k1 = (a.alive && !a.alive[r]) ? a.k0 : a.k1;   // wave-uniform: a dead ray walks nothing
    int n = 0;
    for (int kb = a.k0; kb < k1; kb += 64) {
        const int k = kb + lane;
        bool on = false;
        if (k < k1) {
            float z, p[3];
            on = march_sample(a, m, k, z, p);
        }
        n += __popcll(__ballot(on));
    }
    if (lane == 0) {
        a.counts[r] = n;
        if (a.rays_d) {
            a.rays_d[3 * r] = m.d[0]; a.rays_d[3 * r + 1] = m.d[1]; a.rays_d[3 * r + 2] = m.d[2];
        }
    }
}

// block_counts[b] = the counts of rays [b * kCompactBlock, (b + 1) * kCompactBlock): item = ray, every entry of the
// workspace is written
__global__ void __launch_bounds__(kCompactThreads) march_block_counts_kernel(MarchArgs a) {
    int n = 0;
    for (int k = 0; k < kCompactPer; ++k) {
        const int64_t r = compact_item(k);
        if (r < a.R) n += a.counts[r];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    __shared__ int s[kCompactWaves];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < kCompactWaves; ++i) t += s[i];
        a.block_counts[blockIdx.x] = t;
    }
}

// off = exclusive scan of counts: item = ray, block offsets from compact_common.h, an inclusive wave scan and
// the waves' totals inside each iteration of 256 rays
__global__ void __launch_bounds__(kCompactThreads) march_offsets_kernel(MarchArgs a) {
    int64_t base = compact_block_offset(a.block_counts);
    __shared__ int s_w[kCompactWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = 0; k < kCompactPer; ++k) {
        const int64_t r = compact_item(k);
        const int c = r < a.R ? a.counts[r] : 0;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) s_w[w] = incl;
        __syncthreads();
        int64_t off = base + (incl - c);
        for (int i = 0; i < w; ++i) off += s_w[i];
        if (r < a.R) {
            a.off[r] = (int32_t)off;
            if (r == a.R - 1) a.off[a.R] = (int32_t)(off + c);
        }
        for (int i = 0; i < kCompactWaves; ++i) base += s_w[i];
        __syncthreads();
    }
}

// kRays: the entry's ray index into ray_c instead of the ray's SH4 row into sh_c (<false> is the kernel as it was)
template <bool kRays>
__global__ void __launch_bounds__(kMarchThreads) march_write_kernel(MarchArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kMarchWaves + (threadIdx.x >> 6);
    if (r >= a.R) return;   // wave-uniform
    if (a.counts[r] == 0) return;
    const MarchRay m = march_ray(a, r);
    float sh[16] = {};
    if constexpr (!kRays) {
        if (a.sh_c) {
            const float* v = a.rays + r * a.C + 8;
            sh4_eval(v[0], v[1], v[2], sh);
        }
    }
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int64_t base = a.off[r];
    for (int kb = a.k0; kb < a.k1; kb += 64) {   // a dead ray has counts[r] == 0 and never gets here
        const int k = kb + lane;
        bool on = false;
        float z = 0.f, p[3] = {0.f, 0.f, 0.f};
        if (k < a.k1) on = march_sample(a, m, k, z, p);
        const uint64_t mask = __ballot(on);
        const int64_t idx = base + __popcll(mask & below);
        if (on && idx >= 0 && idx < a.capacity) {
            a.pts_c[3 * idx] = p[0]; a.pts_c[3 * idx + 1] = p[1]; a.pts_c[3 * idx + 2] = p[2];
            a.z_c[idx] = z;
            a.dist_c[idx] = k + 1 < a.K ? march_depth(m, a.t[k + 1]) - z : 1e10f;
            if constexpr (kRays) {
                a.ray_c[idx] = (int32_t)r;
            } else if (a.sh_c) {
                float4* dst = reinterpret_cast<float4*>(a.sh_c + 16 * idx);
#pragma unroll
                for (int q = 0; q < 4; ++q) dst[q] = make_float4(sh[4 * q], sh[4 * q + 1], sh[4 * q + 2], sh[4 * q + 3]);
            }
        }
        base += __popcll(mask);
    }
}

// ---------------------------------------------------------------- the jittered lattice
struct JitterArgs {
    const float* u;          // optional [R, K]: the uniforms
    uint64_t seed, offset;   // else Philox with this pair,
    const uint64_t* rng;     // or with the device pair rng[0], rng[1] if given
};

// sampling.hip's sample_stratified_kernel with lindisp = 0, perturb = 1: the depth of lattice sample k < K of ray r
__device__ __forceinline__ float jitter_depth(const MarchArgs& a, const JitterArgs& j, const MarchRay& m, int64_t r,
                                              int k, uint64_t seed, uint64_t offset) {
    const float z = march_depth(m, a.t[k]);
    const float zl = k > 0 ? march_depth(m, a.t[k - 1]) : 0.f;
    const float zh = k + 1 < a.K ? march_depth(m, a.t[k + 1]) : 0.f;
    const float upper = k + 1 < a.K ? 0.5f * (zh + z) : z;
    const float lower = k > 0 ? 0.5f * (z + zl) : z;
    const int64_t i = r * a.K + k;
    const float u = j.u ? j.u[i] : philox_uniform(seed, offset, (uint64_t)i);
    return lower + (upper - lower) * u;
}

// march_sample at the jittered depth
__device__ __forceinline__ bool jitter_sample(const MarchArgs& a, const JitterArgs& j, const MarchRay& m, int64_t r,
                                              int k, uint64_t seed, uint64_t offset, float& z, float* p) {
    z = jitter_depth(a, j, m, r, k, seed, offset);
    p[0] = m.o[0] + m.d[0] * z;
    p[1] = m.o[1] + m.d[1] * z;
    p[2] = m.o[2] + m.d[2] * z;
    return occ_occupied(a.g, a.bits, p);
}

// march_count_kernel over the whole lattice at the jittered depths
__global__ void __launch_bounds__(kMarchThreads) jitter_count_kernel(MarchArgs a, JitterArgs j) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kMarchWaves + (threadIdx.x >> 6);
    if (r >= a.R) return;   // wave-uniform
    const MarchRay m = march_ray(a, r);
    const uint64_t seed = j.rng ? j.rng[0] : j.seed, offset = j.rng ? j.rng[1] : j.offset;
    int n = 0;
    for (int kb = 0; kb < a.K; kb += 64) {
        const int k = kb + lane;
        bool on = false;
        if (k < a.K) {
            float z, p[3];
            on = jitter_sample(a, j, m, r, k, seed, offset, z, p);
        }
        n += __popcll(__ballot(on));
    }
    if (lane == 0) {
        a.counts[r] = n;
        if (a.rays_d) {
            a.rays_d[3 * r] = m.d[0]; a.rays_d[3 * r + 1] = m.d[1]; a.rays_d[3 * r + 2] = m.d[2];
        }
    }
}

// march_write_kernel over the whole lattice at the jittered depths, one iteration ahead of its stores: dist needs the
// next sample's jittered depth, which lane 63 finds in lane 0 of the iteration ahead
template <bool kRays>
__global__ void __launch_bounds__(kMarchThreads) jitter_write_kernel(MarchArgs a, JitterArgs j) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kMarchWaves + (threadIdx.x >> 6);
    if (r >= a.R) return;   // wave-uniform
    if (a.counts[r] == 0) return;
    const MarchRay m = march_ray(a, r);
    const uint64_t seed = j.rng ? j.rng[0] : j.seed, offset = j.rng ? j.rng[1] : j.offset;
    float sh[16] = {};
    if constexpr (!kRays) {
        const float* v = a.rays + r * a.C + 8;
        sh4_eval(v[0], v[1], v[2], sh);
    }
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int64_t base = a.off[r];
    bool on = false;
    float z = 0.f, p[3] = {0.f, 0.f, 0.f};
    if (lane < a.K) on = jitter_sample(a, j, m, r, lane, seed, offset, z, p);
    for (int kb = 0; kb < a.K; kb += 64) {   // every lane of the wave takes part in the moves below
        const int k = kb + lane;
        bool on_n = false;
        float z_n = 0.f, p_n[3] = {0.f, 0.f, 0.f};
        if (k + 64 < a.K) on_n = jitter_sample(a, j, m, r, k + 64, seed, offset, z_n, p_n);
        const float z_ahead = __shfl(z_n, 0, 64);   // z of lattice index kb + 64 (0.f past the lattice: not used)
        float z_up = __shfl_down(z, 1, 64);
        if (lane == 63) z_up = z_ahead;
        const uint64_t mask = __ballot(on);
        const int64_t idx = base + __popcll(mask & below);
        if (on && idx >= 0 && idx < a.capacity) {
            a.pts_c[3 * idx] = p[0]; a.pts_c[3 * idx + 1] = p[1]; a.pts_c[3 * idx + 2] = p[2];
            a.z_c[idx] = z;
            a.dist_c[idx] = k + 1 < a.K ? z_up - z : 1e10f;
            if constexpr (kRays) {
                a.ray_c[idx] = (int32_t)r;
            } else {
                float4* dst = reinterpret_cast<float4*>(a.sh_c + 16 * idx);
#pragma unroll
                for (int q = 0; q < 4; ++q) dst[q] = make_float4(sh[4 * q], sh[4 * q + 1], sh[4 * q + 2], sh[4 * q + 3]);
            }
        }
        base += __popcll(mask);
        on = on_n; z = z_n; p[0] = p_n[0]; p[1] = p_n[1]; p[2] = p_n[2];
    }
}

// ---------------------------------------------------------------- per-ray SH records
// One thread per packed ray row: sampling.hip's record of the row's view direction (kShRecord floats: the 16 fp32
// coefficients, then pieces 0, 1, 2 of the 16 as bf16), restated
__global__ void __launch_bounds__(256) ray_sh_records_kernel(const float* __restrict__ rays, int64_t R, int C,
                                                             float* __restrict__ rec) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float* v = rays + r * C + 8;
    float o[16];
    sh4_eval(v[0], v[1], v[2], o);
    float4* dst = reinterpret_cast<float4*>(rec + kShRecord * r);
    dst[0] = make_float4(o[0], o[1], o[2], o[3]);
    dst[1] = make_float4(o[4], o[5], o[6], o[7]);
    dst[2] = make_float4(o[8], o[9], o[10], o[11]);
    dst[3] = make_float4(o[12], o[13], o[14], o[15]);
    __bf16* pc = reinterpret_cast<__bf16*>(rec + kShRecord * r + 16);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const __bf16 p0 = (__bf16)o[k];
        const float r1 = o[k] - (float)p0;
        const __bf16 p1 = (__bf16)r1;
        pc[k] = p0;
        pc[16 + k] = p1;
        pc[32 + k] = (__bf16)(r1 - (float)p1);
    }
}

// ---------------------------------------------------------------- packed compositing
struct MarchCompositeArgs {
    const float* raw;        // [n, 4]
    const float* z;          // [n]
    const float* dist;       // [n]
    const int32_t* off;      // [R + 1]
    const float* rays_d;     // [R, 3]
    int64_t R, n;
    int white;
    float* rgb; float* disp; float* acc; float* depth;   // [R, 3], [R], [R], [R]
    float* weights;          // optional [n]
    double* state;           // slabs only: [R, 6] = carry, sum w c (3), sum w, sum w z
    int first, last;         // slabs only: state is not read on first, the maps are written on last
};

// composite_common.h's sigmoidf
__device__ __forceinline__ float march_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// kSlab: one slab of a march in slabs (the state, first and last of the arguments), else the whole list
template <bool kSlab>
__global__ void __launch_bounds__(kMarchThreads) march_composite_kernel(MarchCompositeArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kMarchWaves + (threadIdx.x >> 6);
    if (r >= a.R) return;   // wave-uniform: every lane of a live wave takes part in the scans below
    const float dx = a.rays_d[3 * r], dy = a.rays_d[3 * r + 1], dz = a.rays_d[3 * r + 2];
    const float norm_d = sqrtf(dx * dx + dy * dy + dz * dz);
    // the segment, held inside the list whatever the offsets say
    int64_t end = a.off[r + 1], beg = a.off[r];
    end = end < 0 ? 0 : (end > a.n ? a.n : end);
    beg = beg < 0 ? 0 : (beg > end ? end : beg);
    double carry = 1.0, r0 = 0, r1 = 0, r2 = 0, acc = 0, dn = 0;
    if (kSlab && !a.first) {   // the earlier slabs' sums join lane 0's
        const double* st = a.state + 6 * r;
        carry = st[0];
        if (lane == 0) { r0 = st[1]; r1 = st[2]; r2 = st[3]; acc = st[4]; dn = st[5]; }
    }
    for (int64_t j0 = beg; j0 < end; j0 += 64) {
        const int64_t j = j0 + lane;
        float c0 = 0.f, c1 = 0.f, c2 = 0.f, zj = 0.f, alpha = 0.f, t = 1.f;
        if (j < end) {
            const float4 rw = *reinterpret_cast<const float4*>(a.raw + 4 * j);
            zj = a.z[j];
            const float delta = a.dist[j] * norm_d;
            c0 = march_sigmoid(rw.x); c1 = march_sigmoid(rw.y); c2 = march_sigmoid(rw.z);
            const float sg = rw.w;
            const float relu_s = sg > 0.f ? sg : 0.f;
            const float e = expf(-relu_s * delta);
            alpha = 1.0f - e;
            t = (1.0f - alpha) + 1e-10f;
        }
        const double excl = wave_excl_prod_dpp((double)t);
        const double T = carry * excl;
        const float w = alpha * (float)T;
        carry = carry * readlane_d(excl * (double)t, 63);
        r0 += (double)(w * c0);
        r1 += (double)(w * c1);
        r2 += (double)(w * c2);
        acc += (double)w;
        dn += (double)(w * zj);
        if (a.weights && j < end) a.weights[j] = w;
    }
    const double s0 = wave_sum_dpp(r0), s1 = wave_sum_dpp(r1), s2 = wave_sum_dpp(r2), sa = wave_sum_dpp(acc),
                 sn = wave_sum_dpp(dn);
    if (kSlab && !a.last) {
        if (lane == 0) {
            double* st = a.state + 6 * r;
            st[0] = carry; st[1] = s0; st[2] = s1; st[3] = s2; st[4] = sa; st[5] = sn;
        }
        return;
    }
    float rgb0 = (float)s0, rgb1 = (float)s1, rgb2 = (float)s2;
    const float facc = (float)sa;
    const float num = (float)sn;
    if (lane == 0) {
        const float depth = num / facc;   // NaN at 0 / 0, as ray_sums
        const float mx = (depth != depth) ? depth : fmaxf(1e-10f, depth);
        if (a.white) {
            const float bg = 1.0f - facc;
            rgb0 = rgb0 + bg; rgb1 = rgb1 + bg; rgb2 = rgb2 + bg;
        }
        a.rgb[3 * r] = rgb0; a.rgb[3 * r + 1] = rgb1; a.rgb[3 * r + 2] = rgb2;
        a.acc[r] = facc;
        a.depth[r] = depth;
        if (a.disp) a.disp[r] = 1.0f / mx;
    }
}

// ---------------------------------------------------------------- the stopping rule
// one thread per ray over its segment of the slab's list: early_stop.hip's ert_advance_kernel on packed entries
__global__ void __launch_bounds__(256) march_advance_kernel(const float* __restrict__ raw, const float* __restrict__ dist,
                                                            const int32_t* __restrict__ off,
                                                            const float* __restrict__ rays_d, int64_t R, int64_t n,
                                                            int s1, float tau_max, float* __restrict__ tau,
                                                            uint8_t* __restrict__ alive, int32_t* __restrict__ stop) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R || !alive[r]) return;
    const float dx = rays_d[3 * r + 0], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
    const float norm_d = sqrtf(dx * dx + dy * dy + dz * dz);
    // the segment, held inside the list whatever the offsets say
    int64_t end = off[r + 1], beg = off[r];
    end = end < 0 ? 0 : (end > n ? n : end);
    beg = beg < 0 ? 0 : (beg > end ? end : beg);
    float t = tau[r];
    for (int64_t e = beg; e < end; ++e) {
        const float d = dist[e] * norm_d;
        const float sg = raw[4 * e + 3];
        const float s = sg > 0.f ? sg : 0.f;
        t = t + s * d;
    }
    tau[r] = t;
    if (t > tau_max) {
        alive[r] = 0;
        stop[r] = s1;
    }
}

// the checks the count and the write entries share
static int march_args(MarchArgs& a, const char* what, int64_t n_rays, int n_cols, int64_t n_samples, int64_t k0,
                      int64_t k1, const float* bmin, const float* bmax, int res, bool needs_ws, void* d_workspace,
                      size_t workspace_bytes) {
    int rc = fill_grid(a.g, bmin, bmax, res);
    if (rc) return rc;
    NERF_REQUIRE(n_rays >= 0 && n_rays <= INT32_MAX, "%s: n_rays %lld", what, (long long)n_rays);
    NERF_REQUIRE(n_cols == 8 || n_cols == 11, "%s: ray rows of %d columns (8 or 11)", what, n_cols);
    NERF_REQUIRE(n_samples >= 1 && n_samples <= kMarchMaxSamples, "%s: n_samples %lld (1..%d)", what,
                 (long long)n_samples, kMarchMaxSamples);
    NERF_REQUIRE(n_rays * n_samples <= INT32_MAX, "%s: %lld rays x %lld samples exceed 2^31 - 1; use a smaller chunk",
                 what, (long long)n_rays, (long long)n_samples);
    const size_t need = compact_workspace_bytes(n_rays);
    NERF_REQUIRE(!needs_ws || n_rays == 0 || (d_workspace && workspace_bytes >= need),
                 "%s: null workspace, or workspace %zu B < %zu B", what, workspace_bytes, need);
    NERF_REQUIRE(k0 >= 0 && k0 <= k1 && k1 <= n_samples, "%s: lattice range [%lld, %lld) of %lld samples", what,
                 (long long)k0, (long long)k1, (long long)n_samples);
    a.R = n_rays; a.C = n_cols; a.K = (int)n_samples; a.k0 = (int)k0; a.k1 = (int)k1;
    a.block_counts = needs_ws ? static_cast<int32_t*>(d_workspace) : nullptr;
    return NERF_OK;
}

}  // namespace nerf

using namespace nerf;

extern "C" size_t nerf_march_workspace_bytes(int64_t n_rays) { return compact_workspace_bytes(n_rays); }

// nerf_march_count (0, K, NULL) and nerf_slab_march_count
static int march_count(const char* what, const float* d_rays, int64_t n_rays, int n_cols, const float* d_t,
                       int64_t n_samples, int64_t k0, int64_t k1, const uint8_t* d_alive, const float* bbox_min,
                       const float* bbox_max, int res, const uint32_t* d_bits, int32_t* d_counts, int32_t* d_offsets,
                       float* d_rays_d, void* d_workspace, size_t workspace_bytes, void* stream) {
    MarchArgs a{};
    int rc = march_args(a, what, n_rays, n_cols, n_samples, k0, k1, bbox_min, bbox_max, res, true, d_workspace,
                        workspace_bytes);
    if (rc) return rc;
    if (n_rays == 0) return NERF_OK;
    NERF_REQUIRE(d_rays && d_t && d_bits && d_counts && d_offsets, "%s: null arg", what);
    a.bits = d_bits; a.rays = d_rays; a.t = d_t; a.counts = d_counts; a.off = d_offsets; a.rays_d = d_rays_d;
    a.alive = d_alive;
    hipLaunchKernelGGL(march_count_kernel, dim3(blocks_for(n_rays, kMarchWaves)), dim3(kMarchThreads), 0,
                       as_stream(stream), a);
    const dim3 scan_grid(blocks_for(n_rays, kCompactBlock));
    hipLaunchKernelGGL(march_block_counts_kernel, scan_grid, dim3(kCompactThreads), 0, as_stream(stream), a);
    hipLaunchKernelGGL(march_offsets_kernel, scan_grid, dim3(kCompactThreads), 0, as_stream(stream), a);
    NERF_CHECK_LAUNCH(what);
    return NERF_OK;
}

extern "C" int nerf_march_count(const float* d_rays, int64_t n_rays, int n_cols, const float* d_t, int64_t n_samples,
                                const float* bbox_min, const float* bbox_max, int res, const uint32_t* d_bits,
                                int32_t* d_counts, int32_t* d_offsets, float* d_rays_d, void* d_workspace,
                                size_t workspace_bytes, void* stream) {
    // an n_samples the checks refuse gives the range [0, 0), so that they refuse n_samples and not the range
    return march_count("march_count", d_rays, n_rays, n_cols, d_t, n_samples, 0, n_samples > 0 ? n_samples : 0, nullptr,
                       bbox_min, bbox_max, res, d_bits, d_counts, d_offsets, d_rays_d, d_workspace, workspace_bytes,
                       stream);
}

extern "C" int nerf_slab_march_count(const float* d_rays, int64_t n_rays, int n_cols, const float* d_t,
                                     int64_t n_samples, int64_t k0, int64_t k1, const uint8_t* d_alive,
                                     const float* bbox_min, const float* bbox_max, int res, const uint32_t* d_bits,
                                     int32_t* d_counts, int32_t* d_offsets, float* d_rays_d, void* d_workspace,
                                     size_t workspace_bytes, void* stream) {
    return march_count("slab_march_count", d_rays, n_rays, n_cols, d_t, n_samples, k0, k1, d_alive, bbox_min, bbox_max,
                       res, d_bits, d_counts, d_offsets, d_rays_d, d_workspace, workspace_bytes, stream);
}

// nerf_march_write (0, K) and nerf_slab_march_write; the write needs no alive flags: a dead ray's count is 0
static int march_write(const char* what, const float* d_rays, int64_t n_rays, int n_cols, const float* d_t,
                       int64_t n_samples, int64_t k0, int64_t k1, const float* bbox_min, const float* bbox_max, int res,
                       const uint32_t* d_bits, const int32_t* d_counts, const int32_t* d_offsets, int64_t n_points,
                       int64_t capacity, float* d_pts_c, float* d_z_c, float* d_dist_c, float* d_sh_c, bool index,
                       int32_t* d_ray_c, void* stream) {
    MarchArgs a{};
    int rc = march_args(a, what, n_rays, n_cols, n_samples, k0, k1, bbox_min, bbox_max, res, false, nullptr, 0);
    if (rc) return rc;
    NERF_REQUIRE(n_points >= 0 && n_points <= n_rays * (k1 - k0), "%s: count %lld of %lld lattice samples", what,
                 (long long)n_points, (long long)(n_rays * (k1 - k0)));
    NERF_REQUIRE(capacity >= n_points, "%s: capacity %lld below the count %lld", what, (long long)capacity,
                 (long long)n_points);
    if (n_rays == 0 || n_points == 0) return NERF_OK;
    NERF_REQUIRE(d_rays && d_t && d_bits && d_counts && d_offsets && d_pts_c && d_z_c && d_dist_c, "%s: null arg",
                 what);
    NERF_REQUIRE(!d_sh_c || (n_cols == 11 && ((uintptr_t)d_sh_c & 15) == 0),
                 "%s: SH rows need ray rows of 11 columns and a 16-B aligned sh_c", what);
    NERF_REQUIRE(!index || d_ray_c, "%s: null arg", what);
    a.bits = d_bits; a.rays = d_rays; a.t = d_t; a.counts = const_cast<int32_t*>(d_counts);
    a.off = const_cast<int32_t*>(d_offsets);
    a.capacity = capacity; a.pts_c = d_pts_c; a.z_c = d_z_c; a.dist_c = d_dist_c; a.sh_c = d_sh_c; a.ray_c = d_ray_c;
    const dim3 grid(blocks_for(n_rays, kMarchWaves)), block(kMarchThreads);
    if (index) hipLaunchKernelGGL(march_write_kernel<true>, grid, block, 0, as_stream(stream), a);
    else hipLaunchKernelGGL(march_write_kernel<false>, grid, block, 0, as_stream(stream), a);
    NERF_CHECK_LAUNCH(what);
    return NERF_OK;
}

extern "C" int nerf_march_write(const float* d_rays, int64_t n_rays, int n_cols, const float* d_t, int64_t n_samples,
                                const float* bbox_min, const float* bbox_max, int res, const uint32_t* d_bits,
                                const int32_t* d_counts, const int32_t* d_offsets, int64_t n_points, int64_t capacity,
                                float* d_pts_c, float* d_z_c, float* d_dist_c, float* d_sh_c, void* stream) {
    return march_write("march_write", d_rays, n_rays, n_cols, d_t, n_samples, 0, n_samples > 0 ? n_samples : 0, bbox_min,
                       bbox_max, res, d_bits, d_counts, d_offsets, n_points, capacity, d_pts_c, d_z_c, d_dist_c, d_sh_c,
                       false, nullptr, stream);
}

extern "C" int nerf_slab_march_write(const float* d_rays, int64_t n_rays, int n_cols, const float* d_t,
                                     int64_t n_samples, int64_t k0, int64_t k1, const float* bbox_min,
                                     const float* bbox_max, int res, const uint32_t* d_bits, const int32_t* d_counts,
                                     const int32_t* d_offsets, int64_t n_points, int64_t capacity, float* d_pts_c,
                                     float* d_z_c, float* d_dist_c, float* d_sh_c, void* stream) {
    return march_write("slab_march_write", d_rays, n_rays, n_cols, d_t, n_samples, k0, k1, bbox_min, bbox_max, res,
                       d_bits, d_counts, d_offsets, n_points, capacity, d_pts_c, d_z_c, d_dist_c, d_sh_c, false, nullptr,
                       stream);
}

// the two writes with a ray index in place of the SH rows (march_write_kernel<true>)
extern "C" int nerf_rays_march_write(const float* d_rays, int64_t n_rays, int n_cols, const float* d_t,
                                     int64_t n_samples, const float* bbox_min, const float* bbox_max, int res,
                                     const uint32_t* d_bits, const int32_t* d_counts, const int32_t* d_offsets,
                                     int64_t n_points, int64_t capacity, float* d_pts_c, float* d_z_c, float* d_dist_c,
                                     int32_t* d_ray_c, void* stream) {
    return march_write("rays_march_write", d_rays, n_rays, n_cols, d_t, n_samples, 0, n_samples > 0 ? n_samples : 0,
                       bbox_min, bbox_max, res, d_bits, d_counts, d_offsets, n_points, capacity, d_pts_c, d_z_c,
                       d_dist_c, nullptr, true, d_ray_c, stream);
}

extern "C" int nerf_rays_slab_march_write(const float* d_rays, int64_t n_rays, int n_cols, const float* d_t,
                                          int64_t n_samples, int64_t k0, int64_t k1, const float* bbox_min,
                                          const float* bbox_max, int res, const uint32_t* d_bits,
                                          const int32_t* d_counts, const int32_t* d_offsets, int64_t n_points,
                                          int64_t capacity, float* d_pts_c, float* d_z_c, float* d_dist_c,
                                          int32_t* d_ray_c, void* stream) {
    return march_write("rays_slab_march_write", d_rays, n_rays, n_cols, d_t, n_samples, k0, k1, bbox_min, bbox_max, res,
                       d_bits, d_counts, d_offsets, n_points, capacity, d_pts_c, d_z_c, d_dist_c, nullptr, true, d_ray_c,
                       stream);
}

// the jittered lattice: the two walks over the whole lattice with the sampler's uniforms
static int jitter_uniforms(JitterArgs& j, const char* what, const float* d_u, uint64_t seed, uint64_t offset,
                           const uint64_t* d_rng) {
    NERF_REQUIRE(!d_rng || ((uintptr_t)d_rng & 7) == 0, "%s: the device (seed, offset) pair must be 8-B aligned", what);
    j.u = d_u; j.seed = seed; j.offset = offset; j.rng = d_rng;
    return NERF_OK;
}

extern "C" int nerf_jitter_march_count(const float* d_rays, int64_t n_rays, int n_cols, const float* d_t,
                                       int64_t n_samples, const float* bbox_min, const float* bbox_max, int res,
                                       const uint32_t* d_bits, int32_t* d_counts, int32_t* d_offsets, float* d_rays_d,
                                       void* d_workspace, size_t workspace_bytes, const float* d_u, uint64_t seed,
                                       uint64_t offset, const uint64_t* d_rng, void* stream) {
    const char* what = "jitter_march_count";
    MarchArgs a{};
    JitterArgs j{};
    int rc = march_args(a, what, n_rays, n_cols, n_samples, 0, n_samples > 0 ? n_samples : 0, bbox_min, bbox_max, res,
                        true, d_workspace, workspace_bytes);
    if (rc) return rc;
    if (n_rays == 0) return NERF_OK;
    NERF_REQUIRE(d_rays && d_t && d_bits && d_counts && d_offsets, "%s: null arg", what);
    rc = jitter_uniforms(j, what, d_u, seed, offset, d_rng);
    if (rc) return rc;
    a.bits = d_bits; a.rays = d_rays; a.t = d_t; a.counts = d_counts; a.off = d_offsets; a.rays_d = d_rays_d;
    hipLaunchKernelGGL(jitter_count_kernel, dim3(blocks_for(n_rays, kMarchWaves)), dim3(kMarchThreads), 0,
                       as_stream(stream), a, j);
    const dim3 scan_grid(blocks_for(n_rays, kCompactBlock));
    hipLaunchKernelGGL(march_block_counts_kernel, scan_grid, dim3(kCompactThreads), 0, as_stream(stream), a);
    hipLaunchKernelGGL(march_offsets_kernel, scan_grid, dim3(kCompactThreads), 0, as_stream(stream), a);
    NERF_CHECK_LAUNCH(what);
    return NERF_OK;
}

extern "C" int nerf_jitter_march_write(const float* d_rays, int64_t n_rays, int n_cols, const float* d_t,
                                       int64_t n_samples, const float* bbox_min, const float* bbox_max, int res,
                                       const uint32_t* d_bits, const int32_t* d_counts, const int32_t* d_offsets,
                                       int64_t n_points, int64_t capacity, float* d_pts_c, float* d_z_c,
                                       float* d_dist_c, float* d_sh_c, int32_t* d_ray_c, const float* d_u,
                                       uint64_t seed, uint64_t offset, const uint64_t* d_rng, void* stream) {
    const char* what = "jitter_march_write";
    MarchArgs a{};
    JitterArgs j{};
    int rc = march_args(a, what, n_rays, n_cols, n_samples, 0, n_samples > 0 ? n_samples : 0, bbox_min, bbox_max, res,
                        false, nullptr, 0);
    if (rc) return rc;
    NERF_REQUIRE(n_points >= 0 && n_points <= n_rays * n_samples, "%s: count %lld of %lld lattice samples", what,
                 (long long)n_points, (long long)(n_rays * n_samples));
    NERF_REQUIRE(capacity >= n_points, "%s: capacity %lld below the count %lld", what, (long long)capacity,
                 (long long)n_points);
    if (n_rays == 0) return NERF_OK;
    NERF_REQUIRE((d_sh_c != nullptr) != (d_ray_c != nullptr),
                 "%s: exactly one of sh_c (SH rows) and ray_c (ray indices) must be given", what);
    if (n_points == 0) return NERF_OK;
    NERF_REQUIRE(d_rays && d_t && d_bits && d_counts && d_offsets && d_pts_c && d_z_c && d_dist_c, "%s: null arg",
                 what);
    NERF_REQUIRE(!d_sh_c || (n_cols == 11 && ((uintptr_t)d_sh_c & 15) == 0),
                 "%s: SH rows need ray rows of 11 columns and a 16-B aligned sh_c", what);
    rc = jitter_uniforms(j, what, d_u, seed, offset, d_rng);
    if (rc) return rc;
    a.bits = d_bits; a.rays = d_rays; a.t = d_t; a.counts = const_cast<int32_t*>(d_counts);
    a.off = const_cast<int32_t*>(d_offsets);
    a.capacity = capacity; a.pts_c = d_pts_c; a.z_c = d_z_c; a.dist_c = d_dist_c; a.sh_c = d_sh_c; a.ray_c = d_ray_c;
    const dim3 grid(blocks_for(n_rays, kMarchWaves)), block(kMarchThreads);
    if (d_ray_c) hipLaunchKernelGGL(jitter_write_kernel<true>, grid, block, 0, as_stream(stream), a, j);
    else hipLaunchKernelGGL(jitter_write_kernel<false>, grid, block, 0, as_stream(stream), a, j);
    NERF_CHECK_LAUNCH(what);
    return NERF_OK;
}

// the kShRecord record of every packed ray row's view direction (ray_sh_records_kernel)
extern "C" int nerf_ray_sh_records(const float* d_rays, int64_t n_rays, int n_cols, float* d_sh_rec, void* stream) {
    NERF_REQUIRE(n_rays >= 0, "ray_sh_records: n_rays %lld", (long long)n_rays);
    NERF_REQUIRE(n_cols == 11, "ray_sh_records: ray rows of %d columns (11: the view direction is columns 8..10)",
                 n_cols);
    NERF_REQUIRE((int64_t)kShRecord * n_rays < ((int64_t)1 << 31), "ray_sh_records: %lld rays exceed 32-bit indexing",
                 (long long)n_rays);
    if (n_rays == 0) return NERF_OK;
    NERF_REQUIRE(d_rays && d_sh_rec, "ray_sh_records: null arg");
    NERF_REQUIRE(((uintptr_t)d_sh_rec & 15) == 0, "ray_sh_records: SH records must be 16-B aligned");
    hipLaunchKernelGGL(ray_sh_records_kernel, dim3(blocks_for(n_rays, 256)), dim3(256), 0, as_stream(stream), d_rays,
                       n_rays, n_cols, d_sh_rec);
    NERF_CHECK_LAUNCH("ray_sh_records");
    return NERF_OK;
}

// the checks the two compositing entries and the stopping rule share: the sizes and the packed list
static int march_list_args(const char* what, int64_t n_rays, int64_t n_points) {
    NERF_REQUIRE(n_rays >= 0 && n_rays <= INT32_MAX, "%s: n_rays %lld", what, (long long)n_rays);
    NERF_REQUIRE(n_points >= 0 && n_points <= INT32_MAX && n_points <= n_rays * kMarchMaxSamples,
                 "%s: n_points %lld of %lld rays (at most %d each)", what, (long long)n_points, (long long)n_rays,
                 kMarchMaxSamples);
    return NERF_OK;
}

// nerf_march_composite (state NULL: the whole list) and nerf_slab_march_composite
static int march_composite(const char* what, const float* d_raw, const float* d_z, const float* d_dist,
                           const int32_t* d_offsets, const float* d_rays_d, int64_t n_rays, int64_t n_points,
                           int white_bkgd, bool slab, double* d_state, int first, int last, float* d_rgb, float* d_disp,
                           float* d_acc, float* d_depth, float* d_weights, void* stream) {
    int rc = march_list_args(what, n_rays, n_points);
    if (rc) return rc;
    if (n_rays == 0) return NERF_OK;
    NERF_REQUIRE(d_offsets && d_rays_d && d_rgb && d_acc && d_depth, "%s: null arg", what);
    NERF_REQUIRE(!slab || d_state, "%s: null state", what);
    NERF_REQUIRE(n_points == 0 || (d_raw && d_z && d_dist && ((uintptr_t)d_raw & 15) == 0),
                 "%s: null arg, or raw rows not 16-B aligned", what);
    MarchCompositeArgs a{};
    a.raw = d_raw; a.z = d_z; a.dist = d_dist; a.off = d_offsets; a.rays_d = d_rays_d; a.R = n_rays; a.n = n_points;
    a.white = white_bkgd ? 1 : 0; a.rgb = d_rgb; a.disp = d_disp; a.acc = d_acc; a.depth = d_depth;
    a.weights = d_weights; a.state = d_state; a.first = first ? 1 : 0; a.last = last ? 1 : 0;
    const dim3 grid(blocks_for(n_rays, kMarchWaves)), block(kMarchThreads);
    if (slab) hipLaunchKernelGGL(march_composite_kernel<true>, grid, block, 0, as_stream(stream), a);
    else hipLaunchKernelGGL(march_composite_kernel<false>, grid, block, 0, as_stream(stream), a);
    NERF_CHECK_LAUNCH(what);
    return NERF_OK;
}

extern "C" int nerf_march_composite(const float* d_raw, const float* d_z, const float* d_dist,
                                    const int32_t* d_offsets, const float* d_rays_d, int64_t n_rays, int64_t n_points,
                                    int white_bkgd, float* d_rgb, float* d_disp, float* d_acc, float* d_depth,
                                    float* d_weights, void* stream) {
    return march_composite("march_composite", d_raw, d_z, d_dist, d_offsets, d_rays_d, n_rays, n_points, white_bkgd,
                           false, nullptr, 1, 1, d_rgb, d_disp, d_acc, d_depth, d_weights, stream);
}

extern "C" int nerf_slab_march_composite(const float* d_raw, const float* d_z, const float* d_dist,
                                         const int32_t* d_offsets, const float* d_rays_d, int64_t n_rays,
                                         int64_t n_points, int white_bkgd, double* d_state, int first, int last,
                                         float* d_rgb, float* d_disp, float* d_acc, float* d_depth, float* d_weights,
                                         void* stream) {
    return march_composite("slab_march_composite", d_raw, d_z, d_dist, d_offsets, d_rays_d, n_rays, n_points,
                           white_bkgd, true, d_state, first, last, d_rgb, d_disp, d_acc, d_depth, d_weights, stream);
}

extern "C" int nerf_slab_march_advance(const float* d_raw, const float* d_dist, const int32_t* d_offsets,
                                       const float* d_rays_d, int64_t n_rays, int64_t n_points, int64_t s1,
                                       float tau_max, float* d_tau, uint8_t* d_alive, int32_t* d_stop, void* stream) {
    int rc = march_list_args("slab_march_advance", n_rays, n_points);
    if (rc) return rc;
    NERF_REQUIRE(s1 >= 0 && s1 <= kMarchMaxSamples, "slab_march_advance: slab end %lld (0..%d)", (long long)s1,
                 kMarchMaxSamples);
    NERF_REQUIRE(tau_max > 0.f, "slab_march_advance: tau_max %g must be positive", (double)tau_max);
    if (n_rays == 0) return NERF_OK;
    NERF_REQUIRE(d_offsets && d_rays_d && d_tau && d_alive && d_stop, "slab_march_advance: null arg");
    NERF_REQUIRE(n_points == 0 || (d_raw && d_dist), "slab_march_advance: null arg");
    hipLaunchKernelGGL(march_advance_kernel, dim3(blocks_for(n_rays, 256)), dim3(256), 0, as_stream(stream), d_raw,
                       d_dist, d_offsets, d_rays_d, n_rays, n_points, (int)s1, tau_max, d_tau, d_alive, d_stop);
    NERF_CHECK_LAUNCH("slab_march_advance");
    return NERF_OK;
}
