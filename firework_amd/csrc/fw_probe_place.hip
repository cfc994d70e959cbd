// fw_probe_place.hip — probe relocation and classification for gfx950: the survey of a probe's traced rays, and the step that moves a
// probe out of geometry and marks it active or inactive (include/firework_hip.h has the statement, DESIGN.md §9u the design).  The
// lookups that honour the result are fw_probe_lookup.hip's, over fw_probe_corners.h.
//
//   k_probe_survey             one wave per probe, as k_probe_project.  Lane l walks the rays j = l, l + 64, ... in ascending order: 12 B of
//                              direction, and of the 48-byte hit 4 B of t, 12 B of normal and 4 B of object.  It keeps the nearest back
//                              face and the nearest front face as (dist, j) with strict <, and three counters, all in registers.  The 64
//                              lanes are joined by six __shfl_xor steps that take the lexicographic minimum of (dist, j) and add the
//                              counters; the loop over probes is wave-uniform, so every lane reaches every shuffle.  Lane 0 re-reads the
//                              two winning directions and writes the record as three 16-byte stores.  The minimum and the sums of
//                              integers do not depend on the order they are taken in: the result is a pure function of the inputs.
//   k_probe_relocate_step      one lane per probe: 48 B of survey and 16 B of placement in, 16 B (or, without a move, 4 B) out.
//
// No LDS, no atomics, no barrier, no inline assembly.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.probe_survey and api.probe_relocate_step; fabs is
// exact; sqrt is the device library's float64 function.
#include "fw_probe_place.h"
#include "fw_shared.h"          // grid_for

namespace fw {
namespace {

constexpr int PS_WAVES = 4;                     // waves per workgroup of k_probe_survey
constexpr int PM_BLOCK = 256;                   // k_probe_relocate_step
constexpr uint32_t NO_RAY = 0xFFFFFFFFu;        // no hit of a class yet: above every j (D <= 2^20)

// the nearer of (d, j) and (od, oj): the smaller distance, at equal distance the lower index
__device__ __forceinline__ void take_nearer(double &d, uint32_t &j, double od, uint32_t oj) {
    if (od < d || (od == d && oj < j)) { d = od; j = oj; }
}

__global__ __launch_bounds__(PS_WAVES * 64) void k_probe_survey(uint32_t n_probes, uint32_t directions, const float *__restrict__ rays,
                                                                const uint32_t *__restrict__ hits, float4 *__restrict__ survey) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * PS_WAVES + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * PS_WAVES;
    const double INF = __builtin_huge_val();
    for (uint32_t p = wave; p < n_probes; p += n_waves) {                             // wave-uniform
        const size_t base = (size_t)p * directions;                                   // < 2^31
        double bd = INF, fd = INF;
        uint32_t bj = NO_RAY, fj = NO_RAY, nb = 0u, nf = 0u, nm = 0u;
        for (uint32_t j = lane; j < directions; j += 64u) {
            const float *r = rays + (base + j) * 6u + 3u;
            const uint32_t *h = hits + (base + j) * 12u;
            const float fx = r[0], fy = r[1], fz = r[2];
            if (fx == 0.f && fy == 0.f && fz == 0.f) continue;                        // a ray that was never asked for
            if (h[10] == 0xFFFFFFFFu) { nm++; continue; }
            const double dx = (double)fx, dy = (double)fy, dz = (double)fz;
            const double dist = (double)__uint_as_float(h[0]) * sqrt((dx * dx + dy * dy) + dz * dz);
            const double nx = (double)__uint_as_float(h[4]), ny = (double)__uint_as_float(h[5]), nz = (double)__uint_as_float(h[6]);
            if (((nx * dx + ny * dy) + nz * dz) > 0.0) {
                nb++;
                if (dist < bd) { bd = dist; bj = j; }
            } else {
                nf++;
                if (dist < fd) { fd = dist; fj = j; }
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double obd = __shfl_xor(bd, m, 64), ofd = __shfl_xor(fd, m, 64);
            const uint32_t obj = __shfl_xor(bj, m, 64), ofj = __shfl_xor(fj, m, 64);
            take_nearer(bd, bj, obd, obj);
            take_nearer(fd, fj, ofd, ofj);
            nb += __shfl_xor(nb, m, 64);
            nf += __shfl_xor(nf, m, 64);
            nm += __shfl_xor(nm, m, 64);
        }
        if (lane == 0u) {
            float4 b = make_float4(0.f, 0.f, 0.f, (float)INF), f = b;
            if (bj != NO_RAY) { const float *r = rays + (base + bj) * 6u + 3u; b = make_float4(r[0], r[1], r[2], (float)bd); }
            if (fj != NO_RAY) { const float *r = rays + (base + fj) * 6u + 3u; f = make_float4(r[0], r[1], r[2], (float)fd); }
            float4 *s = survey + (size_t)p * 3u;
            s[0] = b; s[1] = f; s[2] = make_float4((float)nb, (float)nf, (float)nm, 0.f);
        }
    }
}

__global__ __launch_bounds__(PM_BLOCK) void k_probe_relocate_step(DRelocate L, uint32_t n_probes, uint32_t directions,
                                                                  const float4 *__restrict__ survey, float4 *__restrict__ placement, int move) {
    const uint32_t p = blockIdx.x * PM_BLOCK + threadIdx.x;                           // one probe per lane: the grid covers n_probes
    if (p >= n_probes) return;
    const float4 b = survey[(size_t)p * 3u], f = survey[(size_t)p * 3u + 1u], c = survey[(size_t)p * 3u + 2u];
    const bool inside = (double)c.x > L.back_fraction * (double)directions;
    const float a = inside ? 0.f : 1.f;
    if (!move) { ((float *)(placement + p))[3] = a; return; }
    const float4 o = placement[p];
    const double od[3] = {(double)o.x, (double)o.y, (double)o.z};
    double cand[3] = {od[0], od[1], od[2]};
    if (inside) {
        const double dx = (double)b.x, dy = (double)b.y, dz = (double)b.z;
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        const double s = (double)b.w + 0.5 * L.min_front;
        cand[0] = od[0] + (dx / len) * s; cand[1] = od[1] + (dy / len) * s; cand[2] = od[2] + (dz / len) * s;
    } else if (c.y > 0.f && (double)f.w < L.min_front) {
        const double dx = (double)f.x, dy = (double)f.y, dz = (double)f.z;
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        const double s = L.min_front - (double)f.w;
        cand[0] = od[0] - (dx / len) * s; cand[1] = od[1] - (dy / len) * s; cand[2] = od[2] - (dz / len) * s;
    }
    const float cx = (float)cand[0], cy = (float)cand[1], cz = (float)cand[2];
    // rejected, not clamped; a candidate that is not a number is rejected too
    const bool ok = fabs((double)cx) <= L.max_offset[0] && fabs((double)cy) <= L.max_offset[1] && fabs((double)cz) <= L.max_offset[2];
    placement[p] = ok ? make_float4(cx, cy, cz, a) : make_float4(o.x, o.y, o.z, a);
}

} // namespace

void launch_probe_survey(hipStream_t stream, int n_cus, uint32_t n, uint32_t directions, const float *rays, const void *hits, float *survey) {
    hipLaunchKernelGGL(k_probe_survey, dim3(grid_for(n, PS_WAVES, n_cus, 32u)), dim3(PS_WAVES * 64), 0, stream, n, directions, rays,
                       (const uint32_t *)hits, (float4 *)survey);
}

void launch_probe_relocate_step(hipStream_t stream, const DRelocate &rl, uint32_t n, uint32_t directions, const float *survey, float *placement,
                                int move) {
    const uint32_t blocks = (uint32_t)(((uint64_t)n + PM_BLOCK - 1) / PM_BLOCK);
    hipLaunchKernelGGL(k_probe_relocate_step, dim3(blocks), dim3(PM_BLOCK), 0, stream, rl, n, directions, (const float4 *)survey, (float4 *)placement,
                       move);
}

} // namespace fw
