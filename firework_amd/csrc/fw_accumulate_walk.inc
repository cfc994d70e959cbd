// The body of k_accumulate and k_accumulate_adaptive (fw_kernels.hip), included inside both kernels.  (The same body in a device function
// called from both compiled k_accumulate to a different instruction stream; included text compiles to the kernel it was.)
// In scope: DFrame f, sample_rad, accum, moments and constexpr bool MOMENTS.  MOMENTS: accum and moments are whole frames indexed by the
// pixel id of list entry p (f.pixel_ids, or p itself without a list), and each record's square is added to moments.xyz in the same
// pass over the 16-byte records; otherwise accum is indexed by p.
    // linear id of (sample s, pixel p) = s * n_pixels + p = (c * n_waves + w) * 64 + lane -> home = w * cap + c * 64 + lane;
    // one sample further adds n_pixels = 64 * A + B to the linear id: (w, c, lane) are advanced without divisions
    const uint32_t A = f.n_pixels >> 6, B = f.n_pixels & 63u, A_div = A / f.q_n_waves, A_mod = A % f.q_n_waves;
    for (uint32_t p = blockIdx.x * WB + threadIdx.x; p < f.n_pixels; p += gridDim.x * WB) {
        const uint32_t slot = MOMENTS ? (f.pixel_ids ? f.pixel_ids[p] : p) : p;
        float4 a = accum[slot];
        float4 m = MOMENTS ? moments[slot] : make_float4(0.f, 0.f, 0.f, 0.f);
#define FW_ADD(v) do { a.x += (v).x; a.y += (v).y; a.z += (v).z; a.w += (v).w; if (MOMENTS) { m.x += (v).x * (v).x; m.y += (v).y * (v).y; m.z += (v).z * (v).z; } } while (0)
        uint32_t lane = p & 63u, c = (p >> 6) / f.q_n_waves, w = (p >> 6) % f.q_n_waves;
        auto home_then_advance = [&]() {
            const uint32_t home = (w << (f.q_shift + 6u)) | (c << 6) | lane;
            lane += B;
            const uint32_t carry = lane >> 6; lane &= 63u;
            w += A_mod + carry; c += A_div;
            if (w >= f.q_n_waves) { w -= f.q_n_waves; c++; }
            return home;
        };
        uint32_t s = 0;
        if (f.skip_zero_deposits) {
            // black environment: only the slots whose bit is set hold a record (k_shade), all others contribute an exact +0:
            // 1 bit instead of 16 bytes per sample is read, and nobody had to write the zeros
            if (!f.dep_pixel_major) {     // slot-major bits (whole frames): the word of sample s is that of its home slot
                for (; s + 16u <= f.spp_batch; s += 16u) {
                    uint32_t h[16], bw[16];
#pragma unroll
                    for (int k = 0; k < 16; k++) { h[k] = home_then_advance(); bw[k] = f.dep_bits[h[k] >> 5]; }
#pragma unroll
                    for (int k = 0; k < 16; k++) if ((bw[k] >> (h[k] & 31u)) & 1u) { const float4 v = sample_rad[h[k]]; FW_ADD(v); }
                }
                for (; s < f.spp_batch; s++) {
                    const uint32_t h = home_then_advance();
                    if ((f.dep_bits[h >> 5] >> (h & 31u)) & 1u) { const float4 v = sample_rad[h]; FW_ADD(v); }
                }
                accum[slot] = a; if (MOMENTS) moments[slot] = m;
                continue;
            }
            // pixel-major bits (dep_bit_of): the pixel's bits are [p * spp, (p + 1) * spp) — eight words per round trip, then
            // one record per set bit, in sample order
            const uint32_t b0 = p * f.spp_batch, b1 = b0 + f.spp_batch, j_last = (b1 - 1u) >> 5;
            for (uint32_t j0 = b0 >> 5; j0 <= j_last; j0 += 8u) {
                uint32_t wd[8];
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) wd[k] = (j0 + k <= j_last) ? f.dep_bits[j0 + k] : 0u;
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) {
                    const uint32_t j = j0 + k;
                    uint32_t word = wd[k];
                    if (j == (b0 >> 5)) word &= ~0u << (b0 & 31u);
                    if (j == (b1 >> 5)) word &= (1u << (b1 & 31u)) - 1u;
                    while (word) {
                        const uint32_t bit = (uint32_t)__ffs((int)word) - 1u;
                        word &= word - 1u;
                        const uint32_t lin = (j * 32u + bit - b0) * f.n_pixels + p;       // s_local * n_pixels + p
                        const uint32_t g = lin >> 6, cc = g / f.q_n_waves, ww = g - cc * f.q_n_waves;
                        const float4 v = sample_rad[(ww << (f.q_shift + 6u)) | (cc << 6) | (lin & 63u)];
                        FW_ADD(v);
                    }
                }
            }
            accum[slot] = a; if (MOMENTS) moments[slot] = m;
            continue;
        }
        for (; s + 16u <= f.spp_batch; s += 16u) {
            float4 v[16];
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] = sample_rad[home_then_advance()];
#pragma unroll
            for (int k = 0; k < 16; k++) FW_ADD(v[k]);   // render.rs:181: total_color += color(...)
        }
        for (; s < f.spp_batch; s++) {
            float4 v = sample_rad[home_then_advance()];
            FW_ADD(v);
        }
        accum[slot] = a; if (MOMENTS) moments[slot] = m;
    }
#undef FW_ADD
