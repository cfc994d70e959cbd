// fw_reflect.hip — the reflection gather for gfx950: reflection rays drawn from the GGX visible-normal lobe of glossy surface points
// around their view directions, and the reduction of what the rays brought back into the two sums of the estimator F G2 / G1
// (include/firework_hip.h has the statement, DESIGN.md §9za the design).
//
//   k_reflect_rays     k_ao_rays (fw_ao.hip) with the cosine-weighted direction replaced by Heitz's visible normal: one lane per entry
//                      (point q, ray j), id = ids ? ids[first + q] : first + q, position and normal three floats each at id x stride,
//                      the view three floats at id x view_stride, (F0, rho) the float4 spec[id].  The (round, id) shift, the lattice
//                      point (xi1, xi2), the frame of Duff et al. 2017 around the float32 normal made unit in float64 and turned
//                      towards the eye, the sample and its two weights g = G2 / G1 and s = (1 - wo.h)^5 in float64, one rounding to
//                      float32 each; 24 B per ray through LDS — six dword stores per lane at consecutive addresses — and the weights
//                      as one 8 B store per lane.  A dead ray (wi.z <= 0 or wo.z <= 0) and every ray of an unusable point are zeros.
//   k_reflect_reduce   k_gather_reduce's geometry and order (fw_gather.hip): G = the smallest power of two >= min(D, 64) lanes per
//                      point, 64 / G points per wave.  Lane l of a group takes the entries j = l, l + G, ... in ascending order into
//                      eight float64 sums (P.rgb, alive, Q.rgb, sky); an xor butterfly over the distances G/2 .. 1 leaves the same
//                      bits in every lane of the group; lane 0 rounds (1 / D) x each to float32 once and adds them to the point's
//                      running sums, a 32 B record.
//   k_reflect_resolve  one lane per point: (f0 P + Q) / rounds per channel, alive / rounds.
//
// No atomics, no inline assembly; k_reflect_rays alone uses LDS (1536 B) and a barrier.  A point's result depends on no other point and
// not on the launch geometry; two runs are bit-equal.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.reflect_rays / api.reflect_reduce /
// api.reflect_resolve; sin, cos and sqrt are the device library's float64 functions.
#include "fw_reflect.h"
#include "fw_shared.h"

namespace fw {
namespace {

constexpr int RF_BLOCK = 256;
constexpr int RF_WAVES = RF_BLOCK / 64;
constexpr int RR_BLOCK = 64;

__global__ __launch_bounds__(RR_BLOCK) void k_reflect_rays(DReflectRays R, uint32_t n_entries, float *__restrict__ out, float2 *__restrict__ weights) {
    __shared__ float tr[6 * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_chunks = (n_entries + 63u) / 64u;                                    // n_entries < 2^31
    const double Dd = (double)R.directions;
    const double PI = 3.141592653589793, G = 0.6180339887498949;                        // G = (sqrt(5) - 1) / 2, cosine_dir's
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t id0 = c * 64u;
        const uint32_t cnt = min(64u, n_entries - id0);
        if (lane < cnt) {
            const uint32_t i = id0 + lane;
            const uint32_t q = i / R.directions, j = i - q * R.directions;
            const uint32_t id = R.pts.ids ? R.pts.ids[(size_t)R.first + q] : R.first + q;
            double xi_u = 0.5, xi_v = 0.5;
            if (R.jitter) { const Jitter xi = jitter_pair(R.seed32, R.round, id); xi_u = xi.u; xi_v = xi.v; }
            const float *pp = R.pts.positions + (size_t)id * R.pts.stride, *pn = R.pts.normals + (size_t)id * R.pts.stride;
            const float *pv = R.pts.view + (size_t)id * R.pts.view_stride;
            const float px = pp[0], py = pp[1], pz = pp[2], fx = pn[0], fy = pn[1], fz = pn[2], ex = pv[0], ey = pv[1], ez = pv[2];
            const float rho = R.pts.spec[id].w;
            // the lattice point
            const double xi1 = ((double)j + xi_u) / Dd;
            const double tt = (double)j * G + xi_v;
            const double xi2 = tt - floor(tt);
            const double alpha = (double)(rho * rho), a2 = alpha * alpha;
            // the frame
            const double rx = (double)fx, ry = (double)fy, rz = (double)fz, ux = (double)ex, uy = (double)ey, uz = (double)ez;
            const double rl2 = (rx * rx + ry * ry) + rz * rz, ul2 = (ux * ux + uy * uy) + uz * uz;
            const double rl = sqrt(rl2), ul = sqrt(ul2);
            double nx = rx / rl, ny = ry / rl, nz = rz / rl;
            const double wx = -(ux / ul), wy = -(uy / ul), wz = -(uz / ul);
            if ((wx * nx + wy * ny) + wz * nz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
            const double s = copysign(1.0, nz);
            const double a = -1.0 / (s + nz);
            const double b = (nx * ny) * a;
            const double tx = 1.0 + (s * (nx * nx)) * a, ty = s * b, tz = -s * nx;
            const double bx = b, by = s + (ny * ny) * a, bz = -ny;
            const double ox = (wx * tx + wy * ty) + wz * tz, oy = (wx * bx + wy * by) + wz * bz, oz = (wx * nx + wy * ny) + wz * nz;
            // the visible normal
            const double vx = alpha * ox, vy = alpha * oy;
            const double vlen = sqrt((vx * vx + vy * vy) + oz * oz);
            const double vhx = vx / vlen, vhy = vy / vlen, vhz = oz / vlen;
            const double l2 = vhx * vhx + vhy * vhy;
            double t1x = 1.0, t1y = 0.0;
            if (l2 > 0.0) { const double il = 1.0 / sqrt(l2); t1x = -vhy * il; t1y = vhx * il; }
            const double t2x = -(vhz * t1y), t2y = vhz * t1x, t2z = vhx * t1y - vhy * t1x;
            const double sh = 0.5 * (1.0 + vhz);
            const double lo1 = 1.0 + 0.5 * (sqrt(1.0 + a2 * ((ox * ox + oy * oy) / (oz * oz))) - 1.0);
            const double rr = sqrt(xi1);
            const double phi = (2.0 * PI) * xi2;
            const double p1 = rr * cos(phi);
            const double q1 = 1.0 - p1 * p1;
            const double p2 = (1.0 - sh) * sqrt(fmax(q1, 0.0)) + sh * (rr * sin(phi));
            const double pzz = sqrt(fmax(q1 - p2 * p2, 0.0));
            const double nhx = (p1 * t1x + p2 * t2x) + pzz * vhx, nhy = (p1 * t1y + p2 * t2y) + pzz * vhy, nhz = p2 * t2z + pzz * vhz;
            const double gx = alpha * nhx, gy = alpha * nhy, gz = fmax(nhz, 0.0);
            const double hl = sqrt((gx * gx + gy * gy) + gz * gz);
            const double hx = gx / hl, hy = gy / hl, hz = gz / hl;
            const double oh = (ox * hx + oy * hy) + oz * hz;
            const double t2 = 2.0 * oh;
            const double ix = t2 * hx - ox, iy = t2 * hy - oy, iz = t2 * hz - oz;
            const bool usable = finite_f(px) && finite_f(py) && finite_f(pz) && finite_f(fx) && finite_f(fy) && finite_f(fz)
                                && finite_f(ex) && finite_f(ey) && finite_f(ez) && rl2 > 0.0 && ul2 > 0.0 && finite_f(rho) && rho > 0.f;
            const bool alive = usable && iz > 0.0 && oz > 0.0;                            // (a NaN compares false: dead)
            float *d = tr + lane * 6u;
            float2 w = make_float2(0.f, 0.f);
            if (!alive) { d[0] = 0.f; d[1] = 0.f; d[2] = 0.f; d[3] = 0.f; d[4] = 0.f; d[5] = 0.f; }
            else {
                const double li = 0.5 * (sqrt(1.0 + a2 * ((ix * ix + iy * iy) / (iz * iz))) - 1.0);
                const double m = fmax(1.0 - oh, 0.0);
                w = make_float2((float)(lo1 / (lo1 + li)), (float)(((m * m) * (m * m)) * m));
                const double bd = (double)R.bias;
                d[0] = (float)((double)px + bd * nx); d[1] = (float)((double)py + bd * ny); d[2] = (float)((double)pz + bd * nz);
                d[3] = (float)((ix * tx + iy * bx) + iz * nx); d[4] = (float)((ix * ty + iy * by) + iz * ny);
                d[5] = (float)((ix * tz + iy * bz) + iz * nz);
            }
            weights[i] = w;
        }
        __syncthreads();
        float *dst = out + (size_t)id0 * 6u;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) { const uint32_t e = k * 64u + lane; if (e < 6u * cnt) dst[e] = tr[e]; }
        __syncthreads();
    }
}

__global__ __launch_bounds__(RF_BLOCK) void k_reflect_reduce(uint32_t first, uint32_t n, uint32_t directions, uint32_t group,
                                                             const uint32_t *__restrict__ ids, const float4 *__restrict__ surface,
                                                             const float *__restrict__ irradiance, const float *__restrict__ direct,
                                                             const float2 *__restrict__ weights, float *__restrict__ sums) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * RF_WAVES + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * RF_WAVES;
    const uint32_t per = 64u / group, l = lane & (group - 1u), sub = lane / group;
    const double inv_pi = 1.0 / 3.141592653589793;
    const double scale = 1.0 / (double)directions;
    for (uint32_t base = wave * per; base < n; base += n_waves * per) {                   // wave-uniform: every lane reaches the shuffles
        const uint32_t q = base + sub;
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, al = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0, sk = 0.0;
        if (q < n) {
            const size_t e0 = (size_t)q * directions;                                    // < 2^31
            for (uint32_t j = l; j < directions; j += group) {
                const size_t e = e0 + j;
                const float4 a = surface[4 * e], em = surface[4 * e + 3];
                const float2 w = weights[e];
                const float kind = a.w;
                al = al + (w.x > 0.f ? 1.0 : 0.0);
                if (kind == -2.f) continue;                                               // not traced: contributes nothing
                double lr, lg, lb;
                if (kind == -1.f || kind == 3.f) {                                        // the environment, an emitter
                    lr = (double)em.x; lg = (double)em.y; lb = (double)em.z;
                    if (kind == -1.f) sk = sk + 1.0;
                } else {
                    const float *E = irradiance + 3 * e;
                    const float ex = E[0], ey = E[1], ez = E[2];
                    double tr = ex > 0.f ? (double)ex : 0.0, tg = ey > 0.f ? (double)ey : 0.0, tb = ez > 0.f ? (double)ez : 0.0;
                    if (direct) { const float *Ed = direct + 8 * e; tr = tr + (double)Ed[0]; tg = tg + (double)Ed[1]; tb = tb + (double)Ed[2]; }
                    lr = ((double)a.x * tr) * inv_pi; lg = ((double)a.y * tg) * inv_pi; lb = ((double)a.z * tb) * inv_pi;
                }
                const double g = (double)w.x, s = (double)w.y;
                const double wa = g * (1.0 - s), wb = g * s;
                p0 = p0 + wa * lr; p1 = p1 + wa * lg; p2 = p2 + wa * lb;
                q0 = q0 + wb * lr; q1 = q1 + wb * lg; q2 = q2 + wb * lb;
            }
        }
        for (uint32_t m = group >> 1; m >= 1u; m >>= 1) {
            p0 = p0 + __shfl_xor(p0, (int)m, 64); p1 = p1 + __shfl_xor(p1, (int)m, 64); p2 = p2 + __shfl_xor(p2, (int)m, 64);
            al = al + __shfl_xor(al, (int)m, 64);
            q0 = q0 + __shfl_xor(q0, (int)m, 64); q1 = q1 + __shfl_xor(q1, (int)m, 64); q2 = q2 + __shfl_xor(q2, (int)m, 64);
            sk = sk + __shfl_xor(sk, (int)m, 64);
        }
        if (q < n && l == 0u) {
            const uint32_t id = ids ? ids[(size_t)first + q] : first + q;
            float *s = sums + (size_t)id * 8u;
            s[0] = s[0] + (float)(scale * p0); s[1] = s[1] + (float)(scale * p1); s[2] = s[2] + (float)(scale * p2);
            s[3] = s[3] + (float)(scale * al);
            s[4] = s[4] + (float)(scale * q0); s[5] = s[5] + (float)(scale * q1); s[6] = s[6] + (float)(scale * q2);
            s[7] = s[7] + (float)(scale * sk);
        }
    }
}

__global__ __launch_bounds__(RF_BLOCK) void k_reflect_resolve(uint32_t n, double rounds, const uint32_t *__restrict__ ids,
                                                              const float4 *__restrict__ spec, const float4 *__restrict__ sums,
                                                              float4 *__restrict__ out) {
    for (uint32_t q = blockIdx.x * RF_BLOCK + threadIdx.x; q < n; q += gridDim.x * RF_BLOCK) {
        const uint32_t id = ids ? ids[q] : q;
        const float4 p = sums[2 * (size_t)id], qq = sums[2 * (size_t)id + 1], f = spec[id];
        out[id] = make_float4((float)(((double)f.x * (double)p.x + (double)qq.x) / rounds), (float)(((double)f.y * (double)p.y + (double)qq.y) / rounds),
                              (float)(((double)f.z * (double)p.z + (double)qq.z) / rounds), (float)((double)p.w / rounds));
    }
}

} // namespace

void launch_reflect_rays(hipStream_t stream, int n_cus, const DReflectRays &r, uint32_t n, float *rays, float *weights) {
    const uint32_t n_entries = n * r.directions;                              // < 2^31
    hipLaunchKernelGGL(k_reflect_rays, dim3(grid_for(n_entries, 64u, n_cus, 128u)), dim3(RR_BLOCK), 0, stream, r, n_entries, rays, (float2 *)weights);
}

void launch_reflect_reduce(hipStream_t stream, int n_cus, uint32_t first, uint32_t n, uint32_t directions, const uint32_t *ids, const float *surface,
                           const float *irradiance, const float *direct, const float *weights, float *sums) {
    uint32_t group = 1;
    while (group < std::min<uint32_t>(directions, 64u)) group <<= 1;
    const uint32_t per_block = RF_WAVES * (64u / group);
    hipLaunchKernelGGL(k_reflect_reduce, dim3(grid_for(n, per_block, n_cus, 32u)), dim3(RF_BLOCK), 0, stream, first, n, directions, group, ids,
                       (const float4 *)surface, irradiance, direct, (const float2 *)weights, sums);
}

void launch_reflect_resolve(hipStream_t stream, uint32_t n, double rounds, const uint32_t *ids, const float *spec, const float *sums, float *out) {
    hipLaunchKernelGGL(k_reflect_resolve, dim3(grid_for(n, RF_BLOCK, 256, 32u)), dim3(RF_BLOCK), 0, stream, n, rounds, ids, (const float4 *)spec,
                       (const float4 *)sums, (float4 *)out);
}

} // namespace fw
