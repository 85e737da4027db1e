// Lab build only (-DHGX_LAB): a stage of hgx_em.hip's EM driver -- round 2's mid-size reference-order EM (k_em_ref).
// Mid-size problems in the reference's own order of operations: one workgroup, one launch, bit-identical abundances; the kernel
// declines if more than MR_A distinct alleles occur.
int em_lab_mid(const EmCall &e) {
    hgx_classes *c = e.c;
    const int C = c->n_classes;
    if (C > MR_C || c->w64 > 128 || !c->h_rank || hgx_switch_has("em_skip", "exact") || hgx_test_switch("em_no_mid")) return EM_DECLINED;
    OneLaunch o(e);
    DevBuf b_rm, b_km, b_dbg;
    ALLOC(b_rm, (size_t)std::max(C, 1) * MR_AW * 8); ALLOC(b_km, (size_t)MR_A * ((C + 63) / 64) * 8);
    TRY(o.open());
    TRY(o.put_rank());
    TRY(o.zero_state());
    HGX_ONCE_PER_DEVICE({
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_em_ref), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(MrLds)));
    });
    const int max_nnz = hgx_test_switch("em_mid_nnz") ? atoi(hgx_test_switch("em_mid_nnz")) : 65536;
    const bool stamps = hgx_test_switch("mid_stamps") != nullptr;
    if (stamps) ALLOC(b_dbg, 64);
    hipLaunchKernelGGL(k_em_ref, dim3(1), dim3(BLOCK), sizeof(MrLds), e.st, c->d_bits, C, c->w64, o.A, c->d_count, o.len.ptr(), o.b_rank.as<int32_t>(),
                       e.remove_low, b_rm.as<uint64_t>(), b_km.as<uint64_t>(), o.b_out.as<double>(), o.b_scal.as<double>(),
                       o.b_first.as<int32_t>(), max_nnz, b_dbg.as<unsigned long long>());
    if (stamps) {
        unsigned long long h[8] = {0};
        (void)hipStreamSynchronize(e.st);
        (void)hipMemcpy(h, b_dbg.p, 56, hipMemcpyDeviceToHost);
        fprintf(stderr, "[k_em_ref] C %d: set-up %.1f us | rows %.1f | cols %.1f | orders %.1f (%llu derived) | normalise %.1f | sums %.1f\n", C,
                h[0] * 0.01, h[1] * 0.01, h[2] * 0.01, h[3] * 0.01, h[6], h[4] * 0.01, h[5] * 0.01);
    }
    return o.close(true);
}
