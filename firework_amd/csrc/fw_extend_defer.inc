// The body of k_extend_linear_defer<SIMPLE> (fw_kernels.hip: "K2-lin'"), included inside it and inside k_segments_boxlist's scan phase.
// (Text and not a device function for the reason given in fw_shade_nee.inc: included text compiles to the kernel it was.)
// In scope: sc, f, in, hits, segment, n_def (the kernel's arguments, or the fused kernel's variables of those names), bool SIMPLE, and
// wave-uniform uint32_t lane, n (the queue's length), base (the queue's first slot), uint32_t *const L0, *const L1 (the two lists of
// 64 x DEFER_FIELDS dwords in LDS), and scan_objs / scan_cull: sc.obj and sc.obj_cull as the kernel reads them — plain pointers in
// k_extend_linear_defer, ConstQuads (fw_kernels.hip) in the fused kernel.  Leaves both lists empty and every hit record of the queue's n slots stored (not yet acknowledged).
    const float TMIN = 0.001f, TMAX = 2e9f;                          // render.rs:19
    const uint32_t n_first = sc.n_objects - n_def;
    uint32_t cnt0 = 0, cnt1 = 0;
    const RngKey nokey{0, 0, 0};
    auto write_final = [&](uint32_t slot, float t, uint32_t code) {
        if (f.hit4) reinterpret_cast<uint32_t *>(hits)[slot] = code; else qst(&hits[slot], make_float2(t, __uint_as_float(code)));
    };
    auto put = [&](uint32_t *L, uint32_t e, uint32_t sb, float t, uint32_t code, const Ray &r) {
        L[e] = sb; L[64u + e] = __float_as_uint(t); L[128u + e] = code;
        L[192u + e] = __float_as_uint(r.o.x); L[256u + e] = __float_as_uint(r.o.y); L[320u + e] = __float_as_uint(r.o.z);
        L[384u + e] = __float_as_uint(r.d.x); L[448u + e] = __float_as_uint(r.d.y); L[512u + e] = __float_as_uint(r.d.z);
    };
    auto get = [&](const uint32_t *L, uint32_t e, uint32_t &sb, float &t, uint32_t &code, Ray &r) {
        sb = L[e]; t = __uint_as_float(L[64u + e]); code = L[128u + e];
        r.o = mk(__uint_as_float(L[192u + e]), __uint_as_float(L[256u + e]), __uint_as_float(L[320u + e]));
        r.d = mk(__uint_as_float(L[384u + e]), __uint_as_float(L[448u + e]), __uint_as_float(L[512u + e]));
    };
    // the exact test of deferred object d for the first `take` entries of its list, one per lane, the object record wave-uniform
    auto test = [&](uint32_t d, const Ray &r, float &t, uint32_t &code) {
        const uint32_t k = n_first + d;
        const Obj o = load_obj(scan_objs, k);                             // scalar loads
        float tt; uint32_t prim;
        if (hit_rect3d(o.q3, o.q4, to_object_space(o, r), TMIN, t, tt, prim)) { t = tt; code = (k << sc.prim_bits) | prim; }   // a plain Rect3d (the host checks)
    };
    // Lists never overflow: before a chunk appends its candidates, make_room runs whichever list could not take them (and list 1 first when
    // it could not take what list 0's run passes on — the entries flagged in bit 31, counted beforehand).  A run so has between
    // 65 - (the chunk's candidates) and 64 lanes busy.  One textual copy of each run: the two places list 1 may have to run are the two
    // trips of a loop.
    auto append = [&](uint32_t *L, uint32_t &cnt, bool want, uint32_t sb, float t, uint32_t code, const Ray &r) {
        const unsigned long long m = __ballot(want);
        if (!m) return;
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (want) put(L, cnt + rank, sb, t, code, r);
        cnt += (uint32_t)__popcll(m);
    };
    // need0 / need1: entries the caller is about to append to list 0 / list 1 (65: run whatever is there — the end of the queue)
    auto make_room = [&](uint32_t need0, uint32_t need1) {
        const bool r0 = cnt0 != 0u && cnt0 + need0 > 64u;
        const uint32_t pass_on = r0 ? (uint32_t)__popcll(__ballot(lane < cnt0 && (L0[lane] >> 31) != 0u)) : 0u;
#pragma nounroll
        for (int phase = 0; phase < 2; phase++) {
            const bool r1 = cnt1 != 0u && (phase == 0 ? cnt1 + pass_on > 64u : cnt1 + need1 > 64u);
            if (r1) {
                uint32_t sb = 0, code = MISS; float t = TMAX; Ray r{mk(0, 0, 0), mk(0, 0, 1)};
                if (lane < cnt1) { get(L1, lane, sb, t, code, r); test(1, r, t, code); write_final(sb, t, code); }
                cnt1 = 0;
            }
            if (phase == 0 && r0) {
                uint32_t sb = 0, code = MISS; float t = TMAX; Ray r{mk(0, 0, 0), mk(0, 0, 1)};
                const bool on = lane < cnt0;
                if (on) { get(L0, lane, sb, t, code, r); test(0, r, t, code); }
                cnt0 = 0;
                const bool more = on && (sb >> 31) != 0u;              // listed for the second box too
                const uint32_t slot = sb & 0x7fffffffu;
                if (on && !more) write_final(slot, t, code);
                append(L1, cnt1, more, slot, t, code, r);
            }
        }
    };
    float4 ra_n = make_float4(0, 0, 0, 0); float2 rb_n = make_float2(0, 0);
    if (lane < n) { ra_n = qld(&in.ray_a[base + lane]); rb_n = load_ray_b(in, base + lane, f, segment); }
    for (uint32_t c0 = 0; c0 < n; c0 += 64u) {
        const uint32_t j = c0 + lane, i = base + j;
        const float4 ra = ra_n; const float2 rb = rb_n;
        if (j + 64u < n) { ra_n = qld(&in.ray_a[i + 64u]); rb_n = load_ray_b(in, i + 64u, f, segment); }
        const bool active = j < n;
        float best_t = TMAX; uint32_t best_obj = MISS, best_prim = 0;
        bool may0 = false, may1 = false;
        const Ray r = make_ray(ra, rb, f, segment);
        if (active) {
            auto op = scan_objs;
            // A room's walls are PLAIN rectangles (no rotation, no degenerate interval), two or three per axis: they share the reciprocal of
            // their axis' direction component — v_rcp_f32 is a quarter-rate instruction, and the generic test computed it once per rectangle —
            // and skip the generic dispatch.  Wave-uniform branch (the record came through scalar loads); the quotients are hit_rect's, bit for
            // bit.  k_extend 16.2 -> 14.25 ms, cornell 36.0 -> 33.2 ms (gpurun_out/r04y/cornell_rcp.txt).  (The same in the generic linear scans
            // costs them registers they do not have — hdri 7.3 -> 7.8 ms, volume 13.8 -> 15.1 —, and spelled out inside hit_rect3d, where the
            // compiler already shares them, it lost as well: r04y/shared_rcp.txt.)
            const Rcp rcx = make_rcp(r.d.x), rcy = make_rcp(r.d.y), rcz = make_rcp(r.d.z);
            for (uint32_t k = 0; k < n_first; k++, op += OBJ_Q) {
                const Obj o = load_obj(op, 0);
                float t; uint32_t prim = 0; bool h;
                const uint32_t kind = obj_kind(o);
                if (kind >= 1u && kind <= 3u && !(obj_flags(o) & OF_ROTATED) && o.q4.y == 0.f) {
                    const Ray ro{r.o - mk(o.q0.w, o.q1.w, o.q2.w), r.d};                                 // to_object_space without a rotation
                    if (kind == 1u) h = hit_rect_rcp<0>(o.q3.x, o.q3.y, o.q3.z, o.q3.w, o.q4.x, ro, rcz, TMIN, best_t, t);
                    else if (kind == 2u) h = hit_rect_rcp<1>(o.q3.x, o.q3.y, o.q3.z, o.q3.w, o.q4.x, ro, rcy, TMIN, best_t, t);
                    else h = hit_rect_rcp<2>(o.q3.x, o.q3.y, o.q3.z, o.q3.w, o.q4.x, ro, rcx, TMIN, best_t, t);
                } else h = hit_object<false, 0, false, SIMPLE>(sc, o, k, r, TMIN, best_t, nullptr, nokey, segment, t, prim);
                if (h) { best_t = t; best_obj = k; best_prim = prim; }
            }
            // conservative pre-tests, per lane and culled against the hit so far: fw_defer_pretest.h.  The slab test of closest_hit's
            // segment-0 cull (boxes inflated by 1e-4 of the scene and ray-origin scale) with the work moved out of the box loop: the
            // box comes from the host as centre and grown half extent (the second half of obj_cull: nothing wave-uniform is computed
            // here), the reciprocals are the ones the room's rectangles just used (no v_rcp_f32 of its own), a plane pair is three
            // fmas around the centre's distance fma(c, inv, -o * inv), whose rounding the host's extra hundredth of margin covers,
            // and a direction component that is 0, below 2^-40, infinite or NaN lists the ray whatever the slabs say (the exact
            // test accepts t = 0/0).  91 -> 45 vector instructions per chunk for two boxes (profiles/defer_pretest_isa.txt).
            const fwpt::RayTerms rt = fwpt::ray_terms(r.o.x, r.o.y, r.o.z, rcx.r, rcy.r, rcz.r);
            const auto cb = scan_cull + 2 * ((size_t)sc.n_objects + n_first);       // n_def is 1 or 2 (the host: n_defer)
            may0 = fwpt::pretest_fma(rt, cb[0].x, cb[0].y, cb[0].z, cb[1].x, cb[1].y, cb[1].z, best_t);
            if (n_def > 1u) may1 = fwpt::pretest_fma(rt, cb[2].x, cb[2].y, cb[2].z, cb[3].x, cb[3].y, cb[3].z, best_t);
        }
        const uint32_t code = best_obj == MISS ? MISS : ((best_obj << sc.prim_bits) | best_prim);
        const bool c1 = may1 && !may0;                                  // straight to list 1; a ray listed for box 0 carries box 1 in bit 31
        make_room((uint32_t)__popcll(__ballot(may0)), (uint32_t)__popcll(__ballot(c1)));
        if (active && !may0 && !may1) write_final(i, best_t, code);
        append(L0, cnt0, may0, i | (may1 ? 0x80000000u : 0u), best_t, code, r);
        append(L1, cnt1, c1, i, best_t, code, r);
    }
    make_room(65u, 65u);
