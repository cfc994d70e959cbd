// fw_ggx_table.h — what the host runtime (fw_runtime.cpp) and the GGX albedo table's kernels (fw_ggx_table.hip) share.
#pragma once
#include "fw_probe_radiance.h"  // DProbeGrid, DProbeVis, DProbeRadiance

namespace fw {

constexpr uint32_t GGX_MAX_M = 1024;            // fw_ggx_quad: m1 and m2 in 1..1024 (the kernel stages 8 B and 16 B per entry in LDS)
constexpr uint32_t GGX_MIN_N = 2, GGX_MAX_N = 256;   // a table's n_mu and n_rho

// terms (k x 2 floats, 8-byte aligned) of k pairs with the quadrature m1 x m2.  mu and rho not NULL: the pairs are (mu[q], rho[q]),
// q < k.  mu NULL: pair q is the texel first + q of an n_mu x n_rho table, (i, j) = ((first + q) % n_mu, (first + q) / n_mu), at its
// centre float((i + 0.5) / n_mu), float((j + 0.5) / n_rho).  Device memory; one launch on `stream`.
void launch_ggx_terms(hipStream_t stream, int n_cus, uint32_t m1, uint32_t m2, uint32_t k, const float *mu, const float *rho, uint32_t first,
                      uint32_t n_mu, uint32_t n_rho, float *terms);

// terms (k x 2 floats, 8-byte aligned) = the bilinear lookup of table (n_rho x n_mu x 2 floats, 8-byte aligned) at (mu[q], rho[q])
void launch_ggx_table_lookup(hipStream_t stream, uint32_t n_mu, uint32_t n_rho, const float *table, uint32_t k, const float *mu, const float *rho,
                             float *terms);

// The split-sum probe shade of n pixels: launch_probe_shade_glossy's arguments, the table and its sizes, and flags (FW_SPLIT_ENERGY)
void launch_probe_split_shade(hipStream_t stream, const DProbeGrid &g, const DProbeVis *v, const DProbeRadiance &pr, const float *sh, const float *maps,
                              const float *placement, uint32_t n, const float *aov, const float *spec, const float *view, uint32_t view_stride,
                              const float *table, uint32_t n_mu, uint32_t n_rho, uint32_t flags, float gamma, uint8_t *rgb8, float *gamma_rgb,
                              float *linear_rgb);

} // namespace fw
