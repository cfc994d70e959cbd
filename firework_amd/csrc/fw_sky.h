// fw_sky.h — what the host runtime (fw_runtime.cpp) and the sun-and-sky kernels (fw_sky.hip) share: the call's description as the
// kernels read it and the model itself, one statement for the host (fw_sky_sun's T(O)) and the device.  A header of its own, so that the
// translation units of the other .hip files read exactly what they read before.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.sky_radiance; sqrt and exp are the float64 functions of
// whichever side compiles this (the device library's in a kernel, libm's on the host).  Do not reassociate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fw {

// One sky as the kernels read it, formed on the host in float64 from fw_sky's float32 fields (include/firework_hip.h has the statement).
struct DSky {
    double s[3];                // the unit direction towards the sun
    double oy;                  // the observer is (0, oy, 0), oy = Rg + altitude
    double beta_r[3];           // Rayleigh scattering = extinction
    double beta_m, beta_me;     // Mie scattering, and its extinction 1.1 beta_m
    double e0[3];               // sun_irradiance
    double albedo_pi[3];        // ground_albedo / pi
    double et[3];               // E0 T(O): the sun's irradiance at the observer, zeros where the sun is below the observer's horizon
    double cos_sr;              // cos(sun_radius)
    double disc_l[3];           // et / (2 pi (1 - cos_sr)): the disc's radiance for fw_sky_radiance
    uint32_t nv, nl, ss, flags; // view_steps, light_steps, sun_samples, fw_sky.flags
};

// What k_sky_sun needs beside the sky: the rows it visits, its rejection bound and the fallback texel
struct DSkyDisc {
    uint32_t row_lo, row_hi;    // the rows [row_lo, row_hi] lie within sun_radius + pi / H of the sun's: row_lo <= row_hi < H
    double cos_reject;          // a texel whose centre has d . s below this holds no sample inside the disc
    uint32_t fallback;          // env_texel(s): the texel that takes the disc when no sample of any texel lies inside it; < W x H
};

constexpr double SKY_RG = 6360000.0, SKY_RT = 6420000.0, SKY_HR = 7994.0, SKY_HM = 1200.0, SKY_G = 0.76, SKY_PI = 3.141592653589793;

#define FW_SKY_FN __host__ __device__ __forceinline__

FW_SKY_FN double sky_dot(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

// does the ray from P along the unit direction w meet the ground sphere
FW_SKY_FN bool sky_ground(double px, double py, double pz, double wx, double wy, double wz, double &b, double &disc) {
    b = sky_dot(px, py, pz, wx, wy, wz);
    disc = b * b - (sky_dot(px, py, pz, px, py, pz) - SKY_RG * SKY_RG);
    return b < 0.0 && disc > 0.0;
}

// D(P, w, N): the Rayleigh and Mie optical depths (per unit coefficient) from P along w to the top of the atmosphere, N segments with
// quadratic spacing
FW_SKY_FN void sky_depth(double px, double py, double pz, double wx, double wy, double wz, uint32_t n, double &dr, double &dm) {
    const double b = sky_dot(px, py, pz, wx, wy, wz);
    const double tl = -b + sqrt(b * b - (sky_dot(px, py, pz, px, py, pz) - SKY_RT * SKY_RT));
    const double nd = (double)n, nn = (double)(n * n);
    dr = 0.0; dm = 0.0;
    for (uint32_t k = 0; k < n; k++) {
        const double f = ((double)k + 0.5) / nd;
        const double t = tl * (f * f), wd = tl * ((double)(2u * k + 1u) / nn);
        const double qx = px + t * wx, qy = py + t * wy, qz = pz + t * wz;
        const double h = sqrt(sky_dot(qx, qy, qz, qx, qy, qz)) - SKY_RG;
        dr = dr + exp(-h / SKY_HR) * wd;
        dm = dm + exp(-h / SKY_HM) * wd;
    }
}

// T(P) per channel: the sun's transmittance to P, 0 where the ground shadows P
FW_SKY_FN void sky_sun_transmittance(const DSky &K, double px, double py, double pz, double T[3]) {
    double b, disc, lr, lm;
    const bool shadow = sky_ground(px, py, pz, K.s[0], K.s[1], K.s[2], b, disc);
    sky_depth(px, py, pz, K.s[0], K.s[1], K.s[2], K.nl, lr, lm);
    for (int c = 0; c < 3; c++) T[c] = shadow ? 0.0 : exp(-(K.beta_r[c] * lr + K.beta_me * lm));
}

// The radiance that reaches the observer along the unit direction d, without the disc
FW_SKY_FN void sky_radiance(const DSky &K, double dx, double dy, double dz, double L[3]) {
    const double oy = K.oy;
    double bo, dg;
    const bool hit = sky_ground(0.0, oy, 0.0, dx, dy, dz, bo, dg);
    double tmax = -bo + sqrt(bo * bo - (sky_dot(0.0, oy, 0.0, 0.0, oy, 0.0) - SKY_RT * SKY_RT));
    if (hit) tmax = -bo - sqrt(dg);
    const double nd = (double)K.nv, nn = (double)(K.nv * K.nv);
    double o_r = 0.0, o_m = 0.0;
    double sr[3] = {0.0, 0.0, 0.0}, sm[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = 0; i < K.nv; i++) {
        const double f = ((double)i + 0.5) / nd;
        const double t = tmax * (f * f), wd = tmax * ((double)(2u * i + 1u) / nn);
        const double px = 0.0 + t * dx, py = oy + t * dy, pz = 0.0 + t * dz;
        const double h = sqrt(sky_dot(px, py, pz, px, py, pz)) - SKY_RG;
        const double hr = exp(-h / SKY_HR) * wd, hm = exp(-h / SKY_HM) * wd;
        double b, disc, lr, lm;
        const bool shadow = sky_ground(px, py, pz, K.s[0], K.s[1], K.s[2], b, disc);
        sky_depth(px, py, pz, K.s[0], K.s[1], K.s[2], K.nl, lr, lm);
        const double ar = (o_r + 0.5 * hr) + lr, am = (o_m + 0.5 * hm) + lm;
        for (int c = 0; c < 3; c++) {
            const double att = shadow ? 0.0 : exp(-(K.beta_r[c] * ar + K.beta_me * am));
            sr[c] = sr[c] + att * hr;
            sm[c] = sm[c] + att * hm;
        }
        o_r = o_r + hr; o_m = o_m + hm;
    }
    const double mu = sky_dot(dx, dy, dz, K.s[0], K.s[1], K.s[2]);
    const double m1 = 1.0 + mu * mu;
    const double p_r = (3.0 / (16.0 * SKY_PI)) * m1;
    const double x = (1.0 + SKY_G * SKY_G) - (2.0 * SKY_G) * mu;
    const double p_m = ((3.0 / (8.0 * SKY_PI)) * ((1.0 - SKY_G * SKY_G) * m1)) / ((2.0 + SKY_G * SKY_G) * (x * sqrt(x)));
    for (int c = 0; c < 3; c++) L[c] = K.e0[c] * ((sr[c] * K.beta_r[c]) * p_r + (sm[c] * K.beta_m) * p_m);
    if (hit) {
        const double gx = 0.0 + tmax * dx, gy = oy + tmax * dy, gz = 0.0 + tmax * dz;
        const double gl = sqrt(sky_dot(gx, gy, gz, gx, gy, gz));
        const double cg = fmax(sky_dot(gx / gl, gy / gl, gz / gl, K.s[0], K.s[1], K.s[2]), 0.0);
        double T[3];
        sky_sun_transmittance(K, gx, gy, gz, T);
        for (int c = 0; c < 3; c++)
            L[c] = L[c] + (((exp(-(K.beta_r[c] * o_r + K.beta_me * o_m)) * K.albedo_pi[c]) * K.e0[c]) * T[c]) * cg;
    }
}

// the direction of the point (x + fx, j + fy) of a W x H map, fx and fy in (0, 1): panorama_rays' formula
FW_SKY_FN void sky_map_dir(double xf, double jf, double wd, double hd, double &dx, double &dy, double &dz) {
    const double u = xf / wd, v = 1.0 - jf / hd;
    const double phi = SKY_PI - (2.0 * SKY_PI) * u, theta = SKY_PI * v - SKY_PI / 2.0;
    const double ct = cos(theta);
    dx = ct * cos(phi); dy = sin(theta); dz = ct * sin(phi);
}

// k_sky_map: rows [first_row, first_row + n_rows) of the W x H map into out (n_rows x W x 3 floats)
void launch_sky_map(hipStream_t stream, int n_cus, const DSky &sky, uint32_t width, uint32_t height, uint32_t first_row, uint32_t n_rows, float *out);
// k_sky_sun: adds the disc to the texels of the rows [first_row, first_row + n_rows) that it covers; out as launch_sky_map's
void launch_sky_sun(hipStream_t stream, const DSky &sky, const DSkyDisc &disc, uint32_t width, uint32_t height, uint32_t first_row, uint32_t n_rows,
                    float *out);
// k_sky_dirs: out[q] = the radiance along dirs[q x stride .. + 3] for q < n
void launch_sky_dirs(hipStream_t stream, int n_cus, const DSky &sky, uint32_t n, const float *dirs, uint32_t stride, float *out);

} // namespace fw
