// The body of the light-sampling shade kernels k_shade_ls, k_shade_env, k_shade_pl, k_shade_pl_env, k_shade_dl and k_shade_gx_nee (fw_kernels.hip,
// DESIGN §9g-§9i, §9l, §9m),
// included inside each.  (The same body in a __forceinline__ device function called from four thin kernels compiled all 18 instantiations to
// different instruction streams — SGPR spills moved by up to 10 — and shipped kernels keep theirs; included text compiles to the kernel it was.)
// In scope: the kernel's arguments (sc, f, in, out, hits, sample_rad, q, segment, n_mat, n_tex, sh), constexpr (or template parameters)
// int LDS_TAB, MODE (0 or 1: in line; 1: nothing expensive in the scene) and bool ENV, PL, DL, GX, which are shade_path's, and the three pointers
// shade_path takes them with: const DEnvDist *const edp (&ed of the kernel's argument where ENV, else nullptr), const DEmitters *const emp
// (&em where PL, else nullptr) and const DDeltaLights *const dlp (&dl where DL, else nullptr).
// k_shade's loop without the chain state and the list: a light-sampling frame carries the running product and shades in line.
    static_assert(MODE == 0 || MODE == 1, "in line only");
    constexpr bool CHAIN = false;
    const uint32_t w = wave_index(), lane = threadIdx.x & 63u;
#include "fw_shade_tables.inc"
    if (w >= q.n_waves) return;
    const uint32_t n = q.wcount[(size_t)segment * q.n_waves + w];
    const uint32_t base = w * q.cap;
    uint32_t out_n = 0, sh_n = 0;                                        // survivors / shadow rays written so far (wave-uniform)
    PH_DECL;
    float4 ra_n = make_float4(0, 0, 0, 0), st_n = ra_n; float2 rb_n = make_float2(0, 0), hr_n = rb_n; float pb_n = 0.f;
    auto fetch = [&](uint32_t i) {
        ra_n = qld(&in.ray_a[i]); rb_n = load_ray_b(in, i, f, segment); st_n = load_state(in, i, segment); hr_n = qld(&hits[i]);
        pb_n = segment > 0 ? sh.pb_in[i] : 0.f;
    };
    if (lane < n) fetch(base + lane);
    for (uint32_t c0 = 0; c0 < n; c0 += 64u) {
        const uint32_t j = c0 + lane, i = base + j;
        float4 ra = ra_n, st = st_n; float2 rb = rb_n, hr = hr_n;
        LsIO ls{pb_n, 0.f, false, Ray{mk(0, 0, 0), mk(0, 0, 0)}, 0u, mk(0, 0, 0)};
        if (j + 64u < n) fetch(i + 64u);
        bool alive = false;
        Ray nr{mk(0, 0, 0), mk(0, 0, 0)}; V3 nbeta = mk(0, 0, 0); uint32_t path_id = 0, nchain = 0;
        if (j < n) {
            path_id = __float_as_uint(st.w);
            alive = shade_path<MODE != 0, CHAIN, true, ENV, PL, DL, GX>(sc, f, objp, matp, texp, make_ray(ra, rb, f, segment), mk(st.x, st.y, st.z), 0u, path_id, hr.x,
                                                                __float_as_uint(hr.y), segment, sample_rad, nr, nbeta, nchain PH_PASS, nullptr, &sh, &ls, edp, emp, dlp);
        }
        // k_shade's compaction, with p_b next to the state
        const unsigned long long mask = __ballot(alive);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (alive) {
            const uint32_t dst = base + out_n + rank;
            qst(&out.ray_a[dst], make_float4(nr.o.x, nr.o.y, nr.o.z, nr.d.x));
            qst(&out.ray_b[dst], make_float2(nr.d.y, nr.d.z));
            qst(&out.state[dst], make_float4(nbeta.x, nbeta.y, nbeta.z, __uint_as_float(path_id)));
            sh.pb_out[dst] = ls.pb_out;
        }
        if (f.ex.mode) flag_exact(f.ex, alive && needs_exact(f.ex, nr.o.x, nr.o.y, nr.o.z, nr.d.x, nr.d.y, nr.d.z), base + out_n + rank, segment + 1);
        out_n += (uint32_t)__popcll(mask);
        // the shadow rays: the same compaction, into the wave's region of the shadow queue
        const unsigned long long sm = __ballot(ls.shadow);
        if (sm) {
            const uint32_t sr = __builtin_amdgcn_mbcnt_hi((uint32_t)(sm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)sm, 0u));
            if (ls.shadow) {
                const uint32_t d = base + sh_n + sr;
                sh.ray_a[d] = make_float4(ls.sray.o.x, ls.sray.o.y, ls.sray.o.z, ls.sray.d.x);
                sh.ray_b[d] = make_float2(ls.sray.d.y, ls.sray.d.z);
                sh.state[d] = make_float4(ls.pending.x, ls.pending.y, ls.pending.z, __uint_as_float(path_id));
                sh.obj[d] = ls.sobj;
            }
            sh_n += (uint32_t)__popcll(sm);
        }
    }
    if (lane == 0) { q.wcount[(size_t)(segment + 1) * q.n_waves + w] = out_n; sh.wcount[(size_t)(segment + 1) * q.n_waves + w] = sh_n; }
