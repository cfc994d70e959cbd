// fw_probe_radiance.hip — probe radiance maps for gfx950: the reduction of rendered radiance into per-probe octahedral maps, their GGX
// prefilter, the lookup of reflected radiance and the glossy probe shade (include/firework_hip.h has the statement, DESIGN.md §9v the
// design).
//
//   k_probe_radiance_reduce     k_probe_depth's structure with radiance in the place of distance: one workgroup of 256 lanes per probe.
//                               256 directions at a time, lane l turns ray and accum c0 + l (12 B of direction, 16 B of accum) into
//                               (d.xyz, L.rgb) in float64 and stages the 48 B in LDS (12 KB); after the barrier every lane walks the staged
//                               chunk in ascending j for its texels t = lane, lane + 256, ... (at most four, R = 32) with broadcast reads.
//                               A texel's four float64 accumulators stay in registers across the chunks; at the end each is rounded to
//                               float32 once and added to the texel's running sums with one float32 addition.  A texel is one lane's and
//                               its sum is sequential in j: no atomics, no dependence on the launch geometry.
//   k_probe_radiance_prefilter  one workgroup of 256 lanes per probe, grid-stride over probes.  A probe-independent table of the source
//                               texels' (S.xyz, omega) in float64 is computed once per workgroup into LDS (32 B x R^2, 32 KB at R = 32); the
//                               current probe's level 0 is divided out of its sums, written, and staged beside the table as float4 (16 KB).
//                               Lane l owns the output texels l, l + 256 of the levels >= 1 (336 at R = 32, so at most two) and walks the
//                               source in ascending id with broadcast LDS reads, four float64 accumulators per owned texel in registers.
//                               48 KB of static LDS: three workgroups per CU.
//   k_probe_radiance_lookup     one lane per point: the placed lookup's corner weights, then per active corner two bilinear fetches of
//                               four 16-byte texels each.  No LDS, no atomics, no barrier.
//   k_probe_shade_glossy        one lane per pixel: fw_probe_shade_placed's arithmetic where rho is not > 0, else the lookup along the
//                               mirrored view direction under a Schlick Fresnel term.
//
// Every maps index is formed from a clamped cell index and texel indices clamped to [0, R_l - 2] plus 0 or 1, so no load leaves the
// arrays wherever the point lies and whatever the maps hold.  No inline assembly anywhere.
//
// The corner weights, the SH sum and the diffuse shade step are fw_probe_corners.h's (the placed statement: PLACED, with NULL for "no
// placement"); the texel centres, the octahedral fold and the float32 tail are fw_shared.h's.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.probe_radiance_reduce / _prefilter / _lookup; floor,
// min, max and fabs are exact; sqrt is the device library's float64 function.
#include "fw_probe_radiance.h"
#include "fw_probe_corners.h"
#include "fw_probe_radiance_fetch.h"

namespace fw {
namespace {

constexpr int PR_BLOCK = 256;
constexpr int PR_MAXT = 4;                      // reduce: texels per lane at R = 32
constexpr int PF_MAXO = 2;                      // prefilter: output texels per lane at R = 32, four levels (256 + 64 + 16 = 336)
constexpr int PF_MAXSRC = 32 * 32;              // prefilter: source texels at R = 32
constexpr int PL_BLOCK = 256;                   // the lookup and the shade

__global__ __launch_bounds__(PR_BLOCK) void k_probe_radiance_reduce(uint32_t n_probes, uint32_t directions, uint32_t R, uint32_t k, double samples,
                                                                    const float *__restrict__ rays, const float4 *__restrict__ accum,
                                                                    float4 *__restrict__ sums) {
    __shared__ double st[PR_BLOCK * 6];                                                 // (dx, dy, dz, Lr, Lg, Lb) of the staged directions
    const uint32_t lane = threadIdx.x;
    const uint32_t n_tex = R * R;
    const uint32_t nq = (n_tex + PR_BLOCK - 1u) / PR_BLOCK;                             // wave-uniform: 1, or 4 at R = 32
    double T[PR_MAXT][3];
#pragma unroll
    for (int q = 0; q < PR_MAXT; q++) {
        T[q][0] = T[q][1] = T[q][2] = 0.0;
        const uint32_t t = lane + (uint32_t)q * PR_BLOCK;
        if (t < n_tex) texel_dir(t, R, T[q]);
    }
    for (uint32_t p = blockIdx.x; p < n_probes; p += gridDim.x) {
        const size_t base = (size_t)p * directions;                                    // < 2^31
        double A0[PR_MAXT], A1[PR_MAXT], A2[PR_MAXT], W[PR_MAXT];
#pragma unroll
        for (int q = 0; q < PR_MAXT; q++) { A0[q] = 0.0; A1[q] = 0.0; A2[q] = 0.0; W[q] = 0.0; }
        for (uint32_t c0 = 0; c0 < directions; c0 += PR_BLOCK) {
            const uint32_t cnt = min((uint32_t)PR_BLOCK, directions - c0);
            if (lane < cnt) {
                const size_t e = base + c0 + lane;
                const float *r = rays + e * 6u + 3u;
                const float4 a = accum[e];
                double *s = st + lane * 6u;
                s[0] = (double)r[0]; s[1] = (double)r[1]; s[2] = (double)r[2];
                s[3] = (double)a.x / samples; s[4] = (double)a.y / samples; s[5] = (double)a.z / samples;
            }
            __syncthreads();
            for (uint32_t j = 0; j < cnt; j++) {
                const double dx = st[j * 6u], dy = st[j * 6u + 1u], dz = st[j * 6u + 2u];
                const double l0 = st[j * 6u + 3u], l1 = st[j * 6u + 4u], l2 = st[j * 6u + 5u];
#pragma unroll
                for (int q = 0; q < PR_MAXT; q++) {
                    if ((uint32_t)q < nq && lane + (uint32_t)q * PR_BLOCK < n_tex) {
                        double w = fmax(0.0, (T[q][0] * dx + T[q][1] * dy) + T[q][2] * dz);
                        for (uint32_t s = 0; s < k; s++) w = w * w;
                        if (w > 0.0) {                                                  // a ray outside the lobe never touches the texel
                            A0[q] = A0[q] + w * l0;
                            A1[q] = A1[q] + w * l1;
                            A2[q] = A2[q] + w * l2;
                            W[q] = W[q] + w;
                        }
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < PR_MAXT; q++) {
            const uint32_t t = lane + (uint32_t)q * PR_BLOCK;
            if (t < n_tex) {
                float4 *s = sums + ((size_t)p * n_tex + t);                             // < 2^31 texels
                float4 v = *s;
                v.x = v.x + (float)A0[q]; v.y = v.y + (float)A1[q]; v.z = v.z + (float)A2[q]; v.w = v.w + (float)W[q];
                *s = v;
            }
        }
    }
}

__global__ __launch_bounds__(PR_BLOCK) void k_probe_radiance_prefilter(uint32_t n_probes, DProbeRadiance pr, const float4 *__restrict__ sums,
                                                                       float4 *__restrict__ maps) {
    __shared__ double tab[PF_MAXSRC * 4];                                               // (Sx, Sy, Sz, omega) of the source texels: 32 KB
    __shared__ float4 lv0[PF_MAXSRC];                                                   // the current probe's level 0: 16 KB
    const uint32_t lane = threadIdx.x;
    const uint32_t R = pr.R, n_src = R * R, M = pr.texels, n_out = M - n_src;          // n_out <= 336
    const double Rd = (double)R;
    const double cell = 4.0 / (Rd * Rd);
    for (uint32_t s = lane; s < n_src; s += PR_BLOCK) {
        double x, y, z;
        const double len = texel_point(s, R, x, y, z);
        double *e = tab + s * 4u;
        e[0] = x / len; e[1] = y / len; e[2] = z / len;
        e[3] = cell / ((len * len) * len);
    }
    // the lane's output texels o = lane, lane + 256 of the levels >= 1, counted from the start of level 1
    double T[PF_MAXO][3], am1[PF_MAXO], a2[PF_MAXO];
    bool own[PF_MAXO];
#pragma unroll
    for (int q = 0; q < PF_MAXO; q++) {
        T[q][0] = T[q][1] = T[q][2] = 0.0; am1[q] = 0.0; a2[q] = 0.0;
        const uint32_t o = lane + (uint32_t)q * PR_BLOCK;
        own[q] = o < n_out;
        if (own[q]) {
            uint32_t off = 0u;
            for (uint32_t l = 1u; l < pr.levels; l++) {
                const uint32_t Rl = R >> l, nl = Rl * Rl;
                if (o < off + nl) {
                    texel_dir(o - off, Rl, T[q]);
                    const double rho = l == 1u ? pr.rho[1] : (l == 2u ? pr.rho[2] : pr.rho[3]);
                    const double a = rho * rho;
                    a2[q] = a * a;
                    am1[q] = a2[q] - 1.0;
                    break;
                }
                off += nl;
            }
        }
    }
    const bool second = n_out > (uint32_t)PR_BLOCK;                                     // wave-uniform: only R = 32 with four levels
    for (uint32_t p = blockIdx.x; p < n_probes; p += gridDim.x) {
        float4 *__restrict__ out = maps + (size_t)p * M;                                // n_probes x M < 2^31 texels
        const float4 *__restrict__ in = sums + (size_t)p * n_src;
        for (uint32_t s = lane; s < n_src; s += PR_BLOCK) {
            const float4 v = in[s];
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!(v.w == 0.f)) {
                const double W = (double)v.w;
                o.x = (float)((double)v.x / W); o.y = (float)((double)v.y / W); o.z = (float)((double)v.z / W); o.w = 1.f;
            }
            lv0[s] = o;
            out[s] = o;
        }
        __syncthreads();                                                                // the table (first pass) and level 0 are in LDS
        if (n_out > 0u) {
            double A0[PF_MAXO], A1[PF_MAXO], A2[PF_MAXO], Wt[PF_MAXO];
#pragma unroll
            for (int q = 0; q < PF_MAXO; q++) { A0[q] = 0.0; A1[q] = 0.0; A2[q] = 0.0; Wt[q] = 0.0; }
            for (uint32_t s = 0; s < n_src; s++) {
                const float4 L = lv0[s];                                                // broadcast reads: every lane the same address
                if (L.w == 0.f) continue;                                               // workgroup-uniform
                const double Sx = tab[s * 4u], Sy = tab[s * 4u + 1u], Sz = tab[s * 4u + 2u], om = tab[s * 4u + 3u];
                const double l0 = (double)L.x, l1 = (double)L.y, l2 = (double)L.z;
#pragma unroll
                for (int q = 0; q < PF_MAXO; q++) {
                    if ((q == 0 || second) && own[q]) {
                        const double c = (T[q][0] * Sx + T[q][1] * Sy) + T[q][2] * Sz;
                        if (c > 0.0) {
                            const double h = (1.0 + c) * 0.5;
                            const double den = h * am1[q] + 1.0;
                            const double w = ((a2[q] / (den * den)) * c) * om;
                            Wt[q] = Wt[q] + w;
                            A0[q] = A0[q] + w * l0;
                            A1[q] = A1[q] + w * l1;
                            A2[q] = A2[q] + w * l2;
                        }
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < PF_MAXO; q++) {
                if (own[q]) {
                    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (!(Wt[q] == 0.0)) { o.x = (float)(A0[q] / Wt[q]); o.y = (float)(A1[q] / Wt[q]); o.z = (float)(A2[q] / Wt[q]); o.w = 1.f; }
                    out[n_src + lane + (uint32_t)q * PR_BLOCK] = o;                     // < M: own[q]
                }
            }
        }
        __syncthreads();                                                                // level 0 is overwritten by the next probe
    }
}

// Four waves per SIMD, not the five its 90 VGPRs would allow: a point gathers up to 1 KB of texels, and on random points the fifth wave
// costs 0.4 % (profiles/probe_lookup.txt)
template <bool DEPTH>
__global__ __launch_bounds__(PL_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_probe_radiance_lookup(DProbeGrid G, DProbeVis V, DProbeRadiance pr, const float4 *__restrict__ maps,
                                                                    const float *__restrict__ placement, uint32_t n,
                                                                    const float *__restrict__ positions, const float *__restrict__ normals,
                                                                    uint32_t stride, const float *__restrict__ dirs,
                                                                    const float *__restrict__ roughness, float *__restrict__ out) {
    const uint32_t q = blockIdx.x * PL_BLOCK + threadIdx.x;                           // one point per lane: the grid covers n
    if (q < n) {
        const float *pp = positions + (size_t)q * stride, *nn = normals + (size_t)q * stride, *dd = dirs + (size_t)q * 3u;
        const float rough = roughness[q];
        Corners C;
        double E[3];
        float r = 0.f, g = 0.f, b = 0.f;
        if (finite_f(dd[0]) && finite_f(dd[1]) && finite_f(dd[2]) && finite_f(rough) &&
            corner_weights<true, DEPTH>(G, V, placement, pp[0], pp[1], pp[2], nn[0], nn[1], nn[2], C) &&
            corners_radiance(G, C, pr, maps, (double)dd[0], (double)dd[1], (double)dd[2], (double)rough, E)) {
            r = (float)E[0]; g = (float)E[1]; b = (float)E[2];
        }
        float *o = out + (size_t)q * 3u;
        o[0] = r; o[1] = g; o[2] = b;
    }
}

// Schlick's Fresnel term F0 + (1 - F0) m^5, m = 1 - cos, with m^5 formed in float64 and rounded once; where nothing is seen m = 0
struct SchlickTerm {
    static constexpr double UNSEEN = 1.0;
    __device__ __forceinline__ void operator()(double cost, const float4 &sp, float &s0, float &s1, float &s2) const {
        const double m = 1.0 - cost;
        const float Sf = (float)(((m * m) * (m * m)) * m);
        s0 = sp.x + (1.f - sp.x) * Sf; s1 = sp.y + (1.f - sp.y) * Sf; s2 = sp.z + (1.f - sp.z) * Sf;
    }
};

template <bool DEPTH>
__global__ __launch_bounds__(PL_BLOCK) void k_probe_shade_glossy(DProbeGrid G, DProbeVis V, DProbeRadiance pr, ShLookupConst K, const float *__restrict__ sh,
                                                                 const float4 *__restrict__ maps, const float *__restrict__ placement, uint32_t n,
                                                                 const float4 *__restrict__ aov, const float4 *__restrict__ spec,
                                                                 const float *__restrict__ view, uint32_t view_stride, float gamma, uint8_t *rgb8,
                                                                 float *gamma_rgb, float *linear_rgb) {
    const uint32_t p = blockIdx.x * PL_BLOCK + threadIdx.x;                           // one pixel per lane: the grid covers n
    if (p < n) shade_glossy_pixel<DEPTH>(G, V, pr, K, sh, maps, placement, p, aov, spec, view, view_stride, gamma, rgb8, gamma_rgb, linear_rgb, SchlickTerm{});
}

uint32_t rad_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + PL_BLOCK - 1) / PL_BLOCK); }        // n > 0; at most 2^24 blocks

} // namespace

void launch_probe_radiance_reduce(hipStream_t stream, uint32_t n, uint32_t directions, const DProbeRadiance &pr, uint32_t samples, const float *rays,
                                  const float *accum, float *sums) {
    hipLaunchKernelGGL(k_probe_radiance_reduce, dim3(n), dim3(PR_BLOCK), 0, stream, n, directions, pr.R, pr.k, (double)samples, rays,
                       (const float4 *)accum, (float4 *)sums);                          // n < 2^27: one workgroup per probe
}

void launch_probe_radiance_prefilter(hipStream_t stream, int n_cus, uint32_t n, const DProbeRadiance &pr, const float *sums, float *maps) {
    hipLaunchKernelGGL(k_probe_radiance_prefilter, dim3(grid_for(n, 1u, n_cus, 3u)), dim3(PR_BLOCK), 0, stream, n, pr, (const float4 *)sums,
                       (float4 *)maps);                                                 // 48 KB of LDS: three per CU
}

void launch_probe_radiance_lookup(hipStream_t stream, const DProbeGrid &g, const DProbeVis *v, const DProbeRadiance &pr, const float *maps,
                                  const float *placement, uint32_t n, const float *positions, const float *normals, uint32_t stride_floats,
                                  const float *dirs, const float *roughness, float *radiance) {
    if (v) hipLaunchKernelGGL(k_probe_radiance_lookup<true>, dim3(rad_blocks(n)), dim3(PL_BLOCK), 0, stream, g, *v, pr, (const float4 *)maps, placement,
                              n, positions, normals, stride_floats, dirs, roughness, radiance);
    else hipLaunchKernelGGL(k_probe_radiance_lookup<false>, dim3(rad_blocks(n)), dim3(PL_BLOCK), 0, stream, g, DProbeVis{nullptr, 0.0, 0u}, pr,
                            (const float4 *)maps, placement, n, positions, normals, stride_floats, dirs, roughness, radiance);
}

void launch_probe_shade_glossy(hipStream_t stream, const DProbeGrid &g, const DProbeVis *v, const DProbeRadiance &pr, const float *sh,
                               const float *maps, const float *placement, uint32_t n, const float *aov, const float *spec, const float *view,
                               uint32_t view_stride, float gamma, uint8_t *rgb8, float *gamma_rgb, float *linear_rgb) {
    if (v) hipLaunchKernelGGL(k_probe_shade_glossy<true>, dim3(rad_blocks(n)), dim3(PL_BLOCK), 0, stream, g, *v, pr, sh_lookup_const(), sh,
                              (const float4 *)maps, placement, n, (const float4 *)aov, (const float4 *)spec, view, view_stride, gamma, rgb8,
                              gamma_rgb, linear_rgb);
    else hipLaunchKernelGGL(k_probe_shade_glossy<false>, dim3(rad_blocks(n)), dim3(PL_BLOCK), 0, stream, g, DProbeVis{nullptr, 0.0, 0u}, pr,
                            sh_lookup_const(), sh, (const float4 *)maps, placement, n, (const float4 *)aov, (const float4 *)spec, view, view_stride, gamma,
                            rgb8, gamma_rgb, linear_rgb);
}

} // namespace fw