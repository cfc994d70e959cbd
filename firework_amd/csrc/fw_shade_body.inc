// The body of k_shade<LDS_TAB, MODE, CHAIN> (fw_kernels.hip) behind its prologue (fw_shade_tables.inc), included inside it and inside
// k_segments_boxlist's shade phase.  (Text and not a device function for the reason given in fw_shade_nee.inc.)
// In scope: sc, f, in, out, hits, sample_rad, q, segment (the kernel's arguments, or the fused kernel's variables of those names), int
// LDS_TAB, MODE, bool CHAIN, objp / matp / texp (fw_shade_tables.inc), shade_list (MODE 2: 128 uint16_t in LDS), wave-uniform uint32_t
// lane, n (the queue's length), base (the queue's first slot) and uint32_t out_n = 0, which it leaves as the number of survivors
// written to `out` (stored, not yet acknowledged).
    uint32_t list_n = 0;                                                 // MODE 2: entries of shade_list (wave-uniform)
    PH_DECL;
// ---- K7: compaction inside the wave's private queue: ballot -> mbcnt prefix -> dense stores --------
    auto compact = [&](bool alive, const Ray &nr, V3 nbeta, uint32_t nchain, uint32_t path_id, uint32_t c0 = 0xffffffffu) {
        const unsigned long long mask = __ballot(alive);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
#if FW_SHADE_STATIC_STORES
        // Round 5: EVERY lane stores, the dead ones into slots of the wave's own output window that no survivor of this chunk can take and
        // that a later chunk overwrites or nobody reads (position c0 + 64 + lane >= out_n + 64, clamped to the window's last slot, which a
        // survivor reaches only when all 64 lanes survive).  Why: on gfx9 loads and stores share ONE in-order counter (vmcnt), and with the
        // stores behind `if (alive)` — a branch the wave may skip — the compiler cannot know how many of them follow the next chunk's
        // prefetch loads, so the loop-top wait for those loads was `s_waitcnt vmcnt(0)`: every chunk of every wave waited for the L2's
        // acknowledgement of its own stores (54 % of k_shade's wave time in s_waitcnt, profiles/r04z_c2_sq.json).  With a static store count
        // the wait is vmcnt(3): the loads, nothing younger.
        if (c0 != 0xffffffffu) {
#if FW_SHADE_STATIC_STORES == 2     // timing variant: every dead lane into ONE slot (the window's last: no survivor takes it while any lane died) — the waits without the traffic
            const uint32_t dst = base + (alive ? out_n + rank : q.cap - 1u);
#else
            const uint32_t dst = base + (alive ? out_n + rank : min(c0 + 64u + lane, q.cap - 1u));
#endif
            qst(&out.ray_a[dst], make_float4(nr.o.x, nr.o.y, nr.o.z, nr.d.x));
            qst(&out.ray_b[dst], make_float2(nr.d.y, nr.d.z));
            if (CHAIN) qst(&reinterpret_cast<float2 *>(out.state)[dst], make_float2(__uint_as_float(nchain), __uint_as_float(path_id)));
            else qst(&out.state[dst], make_float4(nbeta.x, nbeta.y, nbeta.z, __uint_as_float(path_id)));
        } else
#endif
        if (alive) {
            const uint32_t dst = base + out_n + rank;
            qst(&out.ray_a[dst], make_float4(nr.o.x, nr.o.y, nr.o.z, nr.d.x));
            qst(&out.ray_b[dst], make_float2(nr.d.y, nr.d.z));
            if (CHAIN) qst(&reinterpret_cast<float2 *>(out.state)[dst], make_float2(__uint_as_float(nchain), __uint_as_float(path_id)));
            else qst(&out.state[dst], make_float4(nbeta.x, nbeta.y, nbeta.z, __uint_as_float(path_id)));
        }
        if (f.ex.mode)     // a new ray whose result depends on traversal order: k_extend_exact walks it literally (DExact)
            flag_exact(f.ex, alive && needs_exact(f.ex, nr.o.x, nr.o.y, nr.o.z, nr.d.x, nr.d.y, nr.d.z), base + out_n + rank, segment + 1);
        out_n += (uint32_t)__popcll(mask);
    };
    auto load_st = [&](uint32_t idx) { return CHAIN ? load_state_chain(in, idx, segment) : load_state(in, idx, segment); };
    auto load_hit = [&](uint32_t idx) { return f.hit4 ? make_float2(0.f, __uint_as_float(reinterpret_cast<const uint32_t *>(hits)[idx])) : qld(&hits[idx]); };
    // MODE 2: the last `take` listed paths, one per lane, with the full shading code
    auto run_list = [&](uint32_t take) {
        bool alive = false;
        Ray nr{mk(0, 0, 0), mk(0, 0, 0)}; V3 nbeta = mk(0, 0, 0); uint32_t path_id = 0, nchain = 0;
        if (lane < take) {
            const uint32_t i = base + shade_list[list_n - take + lane];
            const float4 ra = qld(&in.ray_a[i]), st = load_st(i); const float2 rb = load_ray_b(in, i, f, segment), hr = load_hit(i);
            path_id = __float_as_uint(st.w);
            alive = shade_path<false, CHAIN>(sc, f, objp, matp, texp, make_ray(ra, rb, f, segment), mk(st.x, st.y, st.z), __float_as_uint(st.x), path_id, hr.x, __float_as_uint(hr.y), segment, sample_rad, nr, nbeta, nchain PH_PASS);
        }
        list_n -= take;
        compact(alive, nr, nbeta, nchain, path_id);
    };
    // software pipeline: next chunk's ray / state / hit are in flight while the current chunk is shaded
    float4 ra_n = make_float4(0, 0, 0, 0), st_n = ra_n; float2 rb_n = make_float2(0, 0), hr_n = rb_n;
#if FW_SHADE_PIPE
    // Round 5: what the prefetch really needs on gfx9.  Loads and stores share ONE in-order counter (vmcnt): waiting for a load means
    // waiting for everything issued before it, and a wait's immediate is the number of YOUNGER operations that may stay outstanding — which
    // the compiler can only use when that number is the same on every path.  The loop used to issue the next chunk's loads at its top
    // behind `if (j + 64 < n)`, gather the path's pixel id (key_of) in the middle and store the survivors behind `if (alive)`: the gather's
    // wait (vmcnt(0): in-order) completed the prefetch a few hundred instructions after it was issued, and the next top's wait (vmcnt(0):
    // unknown store count) completed the stores — every chunk of every wave sat out an HBM round trip and an L2 write acknowledgement
    // (54 % of the wave time in s_waitcnt at 0.79 instruction issue, profiles/r04z_c2_sq.json; fewer instructions or a deeper prefetch
    // changed nothing: DESIGN §5 rounds 1-4).  Now: (A) the chunk's dependent gathers are issued FIRST (the pixel id), (B) then the next
    // chunk's loads, always the same four instructions (indices clamped to the queue's last entry, and where a stream is not read at all —
    // segment-0 state, ray_b of pinhole camera rays — one hot address stands in), (C) the shading, (D) the stores, every lane
    // (FW_SHADE_STATIC_STORES).  The waits become vmcnt(4) for the gather and vmcnt(3) at the top.
    auto prefetch = [&](uint32_t jn) {       // jn: queue position, clamped by the caller
        const uint32_t in_ = base + jn;
        ra_n = qld(&in.ray_a[in_]);
        rb_n = qld(&in.ray_b[short_rays(f, segment) ? base : in_]);
        if (CHAIN) { const float2 v = qld(&reinterpret_cast<const float2 *>(in.state)[segment == 0 ? base : in_]); st_n = make_float4(v.x, 0.f, 0.f, v.y); }
        else st_n = qld(&in.state[segment == 0 ? base : in_]);
        hr_n = load_hit(in_);
    };
    auto fix_implicit = [&](float4 &st_, float2 &rb_, uint32_t slot) {      // the streams that are not stored at segment 0 (load_state*, load_ray_b)
        if (segment == 0) st_ = CHAIN ? make_float4(0.f, 0.f, 0.f, __uint_as_float(slot)) : make_float4(1.f, 1.f, 1.f, __uint_as_float(slot));
        if (short_rays(f, segment)) rb_ = make_float2(0.f, 0.f);
    };
    if (n) {
        prefetch(min(lane, n - 1u));
        // ... and the loop is entered with the same operations behind the first chunk's loads as every later trip has behind its own: three
        // stores (here into the first 64 output slots, which chunk 0's survivors overwrite or nobody reads) — the wait at the top of the loop
        // is compiled once, for the entry and for the back edge, with the smaller of the two counts
        const uint32_t d0 = base + lane;
        qst(&out.ray_a[d0], make_float4(0.f, 0.f, 0.f, 0.f));
        qst(&out.ray_b[d0], make_float2(0.f, 0.f));
        if (CHAIN) qst(&reinterpret_cast<float2 *>(out.state)[d0], make_float2(0.f, 0.f)); else qst(&out.state[d0], make_float4(0.f, 0.f, 0.f, 0.f));
    }
#else
    if (lane < n) { ra_n = qld(&in.ray_a[base + lane]); rb_n = load_ray_b(in, base + lane, f, segment); st_n = load_st(base + lane); hr_n = load_hit(base + lane); }
#endif
    for (uint32_t c0 = 0; c0 < n; c0 += 64u) {
        const uint32_t j = c0 + lane;
        const uint32_t i = base + j;
        float4 ra = ra_n, st = st_n; float2 rb = rb_n, hr = hr_n;
#if FW_SHADE_PIPE
        fix_implicit(st, rb, i);
        const RngKey key_ = key_of(f, __float_as_uint(st.w));        // (A) the chunk's own gather, before (B) the prefetch
        prefetch(min(j + 64u, n - 1u));
        const RngKey *pre_key = &key_;
#else
        if (j + 64u < n) { ra_n = qld(&in.ray_a[i + 64u]); rb_n = load_ray_b(in, i + 64u, f, segment); st_n = load_st(i + 64u); hr_n = load_hit(i + 64u); }
        const RngKey *pre_key = nullptr;
#endif
        bool alive = false, later = false;
        Ray nr{mk(0, 0, 0), mk(0, 0, 0)}; V3 nbeta = mk(0, 0, 0); uint32_t path_id = 0, nchain = 0;
        if (j < n) {
            PH_T0;
            Ray r = make_ray(ra, rb, f, segment);
            V3 beta = mk(st.x, st.y, st.z);
            path_id = __float_as_uint(st.w);
            const uint32_t hit_code = __float_as_uint(hr.y);
#ifdef FW_ABL_SHADE_COPY     // timing ablation (wrong frames): the queue streams and the compaction alone — every hit path survives unchanged
            alive = hit_code != MISS && segment < 10; nr = r; nbeta = beta; nchain = __float_as_uint(st.x) + (pre_key ? pre_key->pixel & 1u : 0u);
#else
            if (MODE == 2 && expensive_shading(sc, objp, matp, hit_code)) later = true;
            else alive = shade_path<MODE != 0, CHAIN>(sc, f, objp, matp, texp, r, beta, __float_as_uint(st.x), path_id, hr.x, hit_code, segment, sample_rad, nr, nbeta, nchain PH_PASS, pre_key);
#endif
            PH_ADD(0);
        }
        { PH_T0; compact(alive, nr, nbeta, nchain, path_id, c0); PH_ADD(7); }
        if (MODE == 2) {
            const unsigned long long lm = __ballot(later);
            if (lm) {
                const uint32_t lr = __builtin_amdgcn_mbcnt_hi((uint32_t)(lm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lm, 0u));
                if (later) shade_list[list_n + lr] = (uint16_t)j;
                list_n += (uint32_t)__popcll(lm);
                if (list_n >= 64u) run_list(64u);
            }
        }
    }
    if (MODE == 2) while (list_n) run_list(min(list_n, 64u));
