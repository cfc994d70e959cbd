// fw_lightmap.hip — the kernels of the lightmap baker for gfx950 (include/firework_hip.h has the statement, DESIGN.md §9o the design).
//
//   k_lm_cover     one wave per triangle: the lanes stride over the texels of the triangle's UV bounding box (clipped to the image), test
//                  the texel centre against three float64 edge functions and atomicMin the triangle's index into the owner map.  The
//                  minimum is order-free, so the map is a pure function of the inputs.
//   k_lm_texels    one lane per texel: float64 barycentrics of the centre in the owner's UV triangle, the interpolated object-space
//                  position and normal, the placement's transform, one rounding to float32; a 32-byte record per texel.
//   k_lm_rays      one lane per entry (covered texel q, direction j): the (round, texel) shift (integer hashes), the cosine-weighted
//                  Fibonacci direction in float64 rotated into the frame of Duff et al. 2017 around the record's normal, one rounding to
//                  float32; reads 32 B of record per lane (64 consecutive entries share one or two texels), writes 24 B per entry through
//                  LDS as k_probe_rays does: six dword stores per lane at consecutive addresses.
//   k_lm_reduce    G = the smallest power of two >= min(D, 64) lanes per texel, 64 / G texels per wave: lane l of a group takes the
//                  entries j = l, l + G, ... in ascending order into three float64 sums, an xor butterfly over the distances G/2 .. 1
//                  leaves the same bits in every lane of the group, lane 0 rounds to float32 once and adds to the texel's running sum.
//                  No atomics, no LDS, no barrier.
//   k_lm_resolve   irradiance = sums / rounds on covered texels with a = 1, zero elsewhere.
//   k_lm_dilate    one dilation pass, one lane per texel, from one buffer to the other.
//
// The jitter draw, the cosine lattice with its tangent frame (k_ao_rays uses the same) and grid_for are fw_shared.h's.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.Lightmap's numpy statements; sin, cos and sqrt are the
// device library's float64 functions, a few float64 ulps from the host's.
#include "fw_lightmap.h"
#include "fw_shared.h"

namespace fw {
namespace {

constexpr int LM_BLOCK = 256;
constexpr int LM_WAVES = LM_BLOCK / 64;
constexpr int LR_BLOCK = 64;

// the edge function of the header: ((bu - au) (pv - av)) - ((bv - av) (pu - au)), every operation rounded in float64
__device__ __forceinline__ double edge(double au, double av, double bu, double bv, double pu, double pv) {
    return (bu - au) * (pv - av) - (bv - av) * (pu - au);
}

struct UvTri { double au, av, bu, bv, cu, cv; uint32_t i0, i1, i2; };

__device__ __forceinline__ UvTri load_uv(const DLightmapMesh &M, uint32_t t) {
    UvTri T;
    T.i0 = M.indices[(size_t)t * 3u]; T.i1 = M.indices[(size_t)t * 3u + 1u]; T.i2 = M.indices[(size_t)t * 3u + 2u];
    T.au = (double)M.uvs[(size_t)T.i0 * 2u]; T.av = (double)M.uvs[(size_t)T.i0 * 2u + 1u];
    T.bu = (double)M.uvs[(size_t)T.i1 * 2u]; T.bv = (double)M.uvs[(size_t)T.i1 * 2u + 1u];
    T.cu = (double)M.uvs[(size_t)T.i2 * 2u]; T.cv = (double)M.uvs[(size_t)T.i2 * 2u + 1u];
    return T;
}

__global__ __launch_bounds__(LM_BLOCK) void k_lm_cover(DLightmapMesh M, uint32_t *__restrict__ owner) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * LM_WAVES + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * LM_WAVES;
    const double Wd = (double)M.width, Hd = (double)M.height;
    for (uint32_t t = wave; t < M.n_tris; t += n_waves) {
        const UvTri T = load_uv(M, t);
        if (edge(T.au, T.av, T.bu, T.bv, T.cu, T.cv) == 0.0) continue;                   // zero UV area covers nothing
        // the bounding box in texels, one texel wider than the centres need, clipped to the image (the inside test decides)
        const double x0d = floor(fmin(T.au, fmin(T.bu, T.cu)) * Wd - 0.5), x1d = ceil(fmax(T.au, fmax(T.bu, T.cu)) * Wd - 0.5);
        const double y0d = floor((1.0 - fmax(T.av, fmax(T.bv, T.cv))) * Hd - 0.5), y1d = ceil((1.0 - fmin(T.av, fmin(T.bv, T.cv))) * Hd - 0.5);
        if (x1d < 0.0 || y1d < 0.0 || x0d > Wd - 1.0 || y0d > Hd - 1.0) continue;
        const uint32_t x0 = (uint32_t)fmax(x0d, 0.0), x1 = (uint32_t)fmin(x1d, Wd - 1.0);
        const uint32_t y0 = (uint32_t)fmax(y0d, 0.0), y1 = (uint32_t)fmin(y1d, Hd - 1.0);
        const uint32_t bw = x1 - x0 + 1u, total = bw * (y1 - y0 + 1u);                  // <= W x H <= 2^28
        for (uint32_t i = lane; i < total; i += 64u) {
            const uint32_t y = y0 + i / bw, x = x0 + i % bw;
            const double pu = ((double)x + 0.5) / Wd, pv = 1.0 - ((double)y + 0.5) / Hd;
            const double e0 = edge(T.au, T.av, T.bu, T.bv, pu, pv), e1 = edge(T.bu, T.bv, T.cu, T.cv, pu, pv),
                         e2 = edge(T.cu, T.cv, T.au, T.av, pu, pv);
            const bool inside = (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
            if (inside) atomicMin(owner + (size_t)y * M.width + x, t);
        }
    }
}

__global__ __launch_bounds__(LM_BLOCK) void k_lm_texels(DLightmapMesh M, uint32_t *__restrict__ owner, float4 *__restrict__ records) {
    const uint32_t n = M.width * M.height;
    const double Wd = (double)M.width, Hd = (double)M.height;
    for (uint32_t id = blockIdx.x * LM_BLOCK + threadIdx.x; id < n; id += gridDim.x * LM_BLOCK) {
        uint32_t t = owner[id];
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t != LM_NO_OWNER) {
            const UvTri T = load_uv(M, t);
            const uint32_t y = id / M.width, x = id - y * M.width;
            const double pu = ((double)x + 0.5) / Wd, pv = 1.0 - ((double)y + 0.5) / Hd;
            const double area = edge(T.au, T.av, T.bu, T.bv, T.cu, T.cv);
            const double b0 = edge(T.bu, T.bv, T.cu, T.cv, pu, pv) / area, b1 = edge(T.cu, T.cv, T.au, T.av, pu, pv) / area,
                         b2 = edge(T.au, T.av, T.bu, T.bv, pu, pv) / area;
            const float *v0 = M.verts + (size_t)T.i0 * 3u, *v1 = M.verts + (size_t)T.i1 * 3u, *v2 = M.verts + (size_t)T.i2 * 3u;
            double p[3], nn[3];
#pragma unroll
            for (int k = 0; k < 3; k++) p[k] = (b0 * (double)v0[k] + b1 * (double)v1[k]) + b2 * (double)v2[k];
            if (M.normals) {
                const float *n0 = M.normals + (size_t)T.i0 * 3u, *n1 = M.normals + (size_t)T.i1 * 3u, *n2 = M.normals + (size_t)T.i2 * 3u;
#pragma unroll
                for (int k = 0; k < 3; k++) nn[k] = (b0 * (double)n0[k] + b1 * (double)n1[k]) + b2 * (double)n2[k];
            } else {                                                                     // (p0 - p2) x (p1 - p2)
                const double ax = (double)v0[0] - (double)v2[0], ay = (double)v0[1] - (double)v2[1], az = (double)v0[2] - (double)v2[2];
                const double bx = (double)v1[0] - (double)v2[0], by = (double)v1[1] - (double)v2[1], bz = (double)v1[2] - (double)v2[2];
                nn[0] = ay * bz - az * by; nn[1] = az * bx - ax * bz; nn[2] = ax * by - ay * bx;
            }
            const double len = sqrt((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]);
            const bool ok = len > 0.0 && len <= 1.7976931348623157e308;                  // (false for NaN)
            nn[0] = nn[0] / len; nn[1] = nn[1] / len; nn[2] = nn[2] / len;
            double wp[3] = {p[0], p[1], p[2]}, wn[3] = {nn[0], nn[1], nn[2]};
            if (M.rotated) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    wp[k] = ((double)M.rows[k][0] * p[0] + (double)M.rows[k][1] * p[1]) + (double)M.rows[k][2] * p[2];
                    wn[k] = ((double)M.rows[k][0] * nn[0] + (double)M.rows[k][1] * nn[1]) + (double)M.rows[k][2] * nn[2];
                }
            }
#pragma unroll
            for (int k = 0; k < 3; k++) { wp[k] = wp[k] + (double)M.position[k]; if (M.negate) wn[k] = -wn[k]; }
            const float fp[3] = {(float)wp[0], (float)wp[1], (float)wp[2]}, fn[3] = {(float)wn[0], (float)wn[1], (float)wn[2]};
            const float big = fmaxf(fmaxf(fmaxf(fabsf(fp[0]), fabsf(fp[1])), fmaxf(fabsf(fp[2]), fabsf(fn[0]))), fmaxf(fabsf(fn[1]), fabsf(fn[2])));
            const bool finite = !(fp[0] != fp[0] || fp[1] != fp[1] || fp[2] != fp[2] || fn[0] != fn[0] || fn[1] != fn[1] || fn[2] != fn[2]);
            if (ok && finite && big <= 3.4028234663852886e38f) {                         // every component finite
                r0 = make_float4(fp[0], fp[1], fp[2], __uint_as_float(t));
                r1 = make_float4(fn[0], fn[1], fn[2], 0.f);
            } else {
                t = LM_NO_OWNER;
                owner[id] = LM_NO_OWNER;
            }
        }
        if (t == LM_NO_OWNER) r0.w = __uint_as_float(LM_NO_OWNER);
        records[(size_t)id * 2u] = r0;
        records[(size_t)id * 2u + 1u] = r1;
    }
}

__global__ __launch_bounds__(LR_BLOCK) void k_lm_rays(DLightmapRays R, uint32_t n_entries, float *__restrict__ out) {
    __shared__ float tr[6 * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_chunks = (n_entries + 63u) / 64u;                                    // n_entries < 2^31
    const double Dd = (double)R.directions;
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t id0 = c * 64u;
        const uint32_t cnt = min(64u, n_entries - id0);
        if (lane < cnt) {
            const uint32_t i = id0 + lane;
            const uint32_t q = i / R.directions, j = i - q * R.directions;
            const uint32_t texel = R.texel_ids[q];                                        // 2 texel + 1 < 2^32: W x H <= 2^28
            double xi_u = 0.5, xi_v = 0.5;
            if (R.jitter) { const Jitter xi = jitter_pair(R.seed32, R.round, texel); xi_u = xi.u; xi_v = xi.v; }
            const float4 rp = R.records[(size_t)texel * 2u], rn = R.records[(size_t)texel * 2u + 1u];
            const CosineDir cd = cosine_dir(j, Dd, xi_u, xi_v, rn.x, rn.y, rn.z);
            float *d = tr + lane * 6u;
            if (R.bias == 0.f) { d[0] = rp.x; d[1] = rp.y; d[2] = rp.z; }
            else {
                const double bd = (double)R.bias;
                d[0] = (float)((double)rp.x + bd * cd.nx); d[1] = (float)((double)rp.y + bd * cd.ny); d[2] = (float)((double)rp.z + bd * cd.nz);
            }
            d[3] = (float)cd.dx; d[4] = (float)cd.dy; d[5] = (float)cd.dz;
        }
        __syncthreads();
        float *dst = out + (size_t)id0 * 6u;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) { const uint32_t e = k * 64u + lane; if (e < 6u * cnt) dst[e] = tr[e]; }
        __syncthreads();
    }
}

__global__ __launch_bounds__(LM_BLOCK) void k_lm_reduce(uint32_t n, uint32_t directions, uint32_t samples, uint32_t group,
                                                        const uint32_t *__restrict__ texel_ids, const float4 *__restrict__ accum,
                                                        float *__restrict__ sums) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * LM_WAVES + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * LM_WAVES;
    const uint32_t per = 64u / group, l = lane & (group - 1u), sub = lane / group;
    const double Sd = (double)samples;
    const double scale = 3.141592653589793 / (double)directions;
    for (uint32_t base = wave * per; base < n; base += n_waves * per) {                   // wave-uniform: every lane reaches the shuffles
        const uint32_t q = base + sub;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (q < n) {
            const float4 *a = accum + (size_t)q * directions;
            for (uint32_t j = l; j < directions; j += group) {
                const float4 v = a[j];
                s0 = s0 + (double)v.x / Sd; s1 = s1 + (double)v.y / Sd; s2 = s2 + (double)v.z / Sd;
            }
        }
        for (uint32_t m = group >> 1; m >= 1u; m >>= 1) {
            s0 = s0 + __shfl_xor(s0, (int)m, 64); s1 = s1 + __shfl_xor(s1, (int)m, 64); s2 = s2 + __shfl_xor(s2, (int)m, 64);
        }
        if (q < n && l == 0u) {
            float *s = sums + (size_t)(texel_ids ? texel_ids[q] : q) * 4u;
            s[0] = s[0] + (float)(scale * s0); s[1] = s[1] + (float)(scale * s1); s[2] = s[2] + (float)(scale * s2);
        }
    }
}

__global__ __launch_bounds__(LM_BLOCK) void k_lm_resolve(uint32_t n, double rounds, const uint32_t *__restrict__ owner,
                                                         const float4 *__restrict__ sums, float4 *__restrict__ out) {
    for (uint32_t id = blockIdx.x * LM_BLOCK + threadIdx.x; id < n; id += gridDim.x * LM_BLOCK) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (owner[id] != LM_NO_OWNER) {
            const float4 s = sums[id];
            o = make_float4((float)((double)s.x / rounds), (float)((double)s.y / rounds), (float)((double)s.z / rounds), 1.f);
        }
        out[id] = o;
    }
}

__global__ __launch_bounds__(LM_BLOCK) void k_lm_dilate(uint32_t width, uint32_t height, const float4 *__restrict__ in, float4 *__restrict__ out) {
    const uint32_t n = width * height;
    for (uint32_t id = blockIdx.x * LM_BLOCK + threadIdx.x; id < n; id += gridDim.x * LM_BLOCK) {
        float4 o = in[id];
        if (!(o.w > 0.f)) {
            const int y = (int)(id / width), x = (int)(id - (uint32_t)y * width);
            float r = 0.f, g = 0.f, b = 0.f;
            uint32_t cnt = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    if (dy == 0 && dx == 0) continue;
                    const int yy = y + dy, xx = x + dx;
                    if (yy < 0 || xx < 0 || yy >= (int)height || xx >= (int)width) continue;
                    const float4 v = in[(size_t)yy * width + (uint32_t)xx];
                    if (v.w > 0.f) { r = r + v.x; g = g + v.y; b = b + v.z; cnt++; }
                }
            }
            if (cnt) { const float c = (float)cnt; o = make_float4(r / c, g / c, b / c, 0.5f); }
        }
        out[id] = o;
    }
}

} // namespace

void launch_lm_cover(hipStream_t stream, int n_cus, const DLightmapMesh &m, uint32_t *owner) {
    hipLaunchKernelGGL(k_lm_cover, dim3(grid_for(m.n_tris, LM_WAVES, n_cus, 32u)), dim3(LM_BLOCK), 0, stream, m, owner);
}

void launch_lm_texels(hipStream_t stream, int n_cus, const DLightmapMesh &m, uint32_t *owner, float4 *records) {
    hipLaunchKernelGGL(k_lm_texels, dim3(grid_for((uint64_t)m.width * m.height, LM_BLOCK, n_cus, 32u)), dim3(LM_BLOCK), 0, stream, m, owner, records);
}

void launch_lm_rays(hipStream_t stream, int n_cus, const DLightmapRays &r, uint32_t n, float *out) {
    const uint32_t n_entries = n * r.directions;                              // < 2^31
    hipLaunchKernelGGL(k_lm_rays, dim3(grid_for(n_entries, 64u, n_cus, 128u)), dim3(LR_BLOCK), 0, stream, r, n_entries, out);
}

void launch_lm_reduce(hipStream_t stream, int n_cus, uint32_t n, uint32_t directions, uint32_t samples, const uint32_t *texel_ids,
                      const float *accum, float *sums) {
    uint32_t group = 1;
    while (group < std::min<uint32_t>(directions, 64u)) group <<= 1;
    const uint32_t per_block = LM_WAVES * (64u / group);
    hipLaunchKernelGGL(k_lm_reduce, dim3(grid_for(n, per_block, n_cus, 32u)), dim3(LM_BLOCK), 0, stream, n, directions, samples, group, texel_ids,
                       (const float4 *)accum, sums);
}

void launch_lm_resolve(hipStream_t stream, uint32_t n_texels, double rounds, const uint32_t *owner, const float *sums, float *out) {
    hipLaunchKernelGGL(k_lm_resolve, dim3(grid_for(n_texels, LM_BLOCK, 256, 32u)), dim3(LM_BLOCK), 0, stream, n_texels, rounds, owner,
                       (const float4 *)sums, (float4 *)out);
}

void launch_lm_dilate(hipStream_t stream, uint32_t width, uint32_t height, const float *in, float *out) {
    hipLaunchKernelGGL(k_lm_dilate, dim3(grid_for((uint64_t)width * height, LM_BLOCK, 256, 32u)), dim3(LM_BLOCK), 0, stream, width, height,
                       (const float4 *)in, (float4 *)out);
}

} // namespace fw
