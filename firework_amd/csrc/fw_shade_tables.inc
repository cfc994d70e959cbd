// The prologue of k_shade and of the light-sampling shade kernels (fw_shade_nee.inc), included inside them: the scene's tables staged in
// LDS.  (Text and not a device function for the reason given in fw_shade_nee.inc: included text compiles to the kernel it was.)
// In scope: DScene sc, uint32_t n_mat, n_tex, and constexpr (or template parameters) int LDS_TAB, MODE and bool CHAIN.
// Leaves objp / matp / texp pointing at the tables shade_path is to read: 1 objects + materials + textures in lds_tables, 2 materials +
// textures only, 0 the resident ones; and the Perlin permutation table in LDS where the kernel can reach such a texture (stage_perm).
// Every thread of the workgroup passes here (__syncthreads): before any `return`.
    const float4 *objp = sc.obj, *matp = sc.mat, *texp = sc.tex;
    if (sc.has_perlin && MODE != 1 && !CHAIN) { stage_perm(); if (!LDS_TAB) __syncthreads(); }
    if (LDS_TAB) {
        const uint32_t no = LDS_TAB == 1 ? sc.n_objects * OBJ_Q : 0u, nm = 2 * n_mat, nt = 2 * n_tex;
        if (LDS_TAB == 1) for (uint32_t k = threadIdx.x; k < no; k += WB) lds_tables[k] = sc.obj[k];
        for (uint32_t k = threadIdx.x; k < nm; k += WB) lds_tables[no + k] = sc.mat[k];
        for (uint32_t k = threadIdx.x; k < nt; k += WB) lds_tables[no + nm + k] = sc.tex[k];
        __syncthreads();
        if (LDS_TAB == 1) objp = lds_tables;
        matp = lds_tables + no; texp = lds_tables + no + nm;
    }
