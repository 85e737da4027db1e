// Lab build only (-DHGX_LAB): a stage of hgx_em.hip's EM driver -- round 1's one-workgroup EM (k_em_small): one launch, one sync.

// k_em_small does not carry the first-class information: looked up for the survivors afterwards
int first_for_present(const EmCall &e) {
    if (!e.first) return HGX_OK;
    std::vector<int32_t> al;
    for (int a = 0; a < e.n_alleles; ++a) if (e.prob[a] >= 0.0) al.push_back(a);
    if (al.empty()) return HGX_OK;
    std::vector<int32_t> f(al.size());
    TRY(hgx_first_classes(e.c, al.data(), (int32_t)al.size(), f.data(), e.st));
    for (size_t i = 0; i < al.size(); ++i) e.first[al[i]] = f[i];
    return HGX_OK;
}

int em_lab_small(const EmCall &e) {
    hgx_classes *c = e.c;
    const int C = c->n_classes;
    if (C > SMALL_C || c->a_pad > EPT * BLOCK || hgx_test_switch("em_no_small")) return EM_DECLINED;
    OneLaunch o(e);
    TRY(o.open());                     // (the kernel writes every state word the host reads: nothing to zero)
    const size_t lds = (size_t)C * c->w64 * 8;
    HGX_ONCE_PER_DEVICE({
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_em_small), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   SMALL_C * (EPT * BLOCK / 64) * 8));
    });
    hipLaunchKernelGGL(k_em_small, dim3(1), dim3(BLOCK), lds, e.st, c->d_bits, C, c->w64, o.A, c->d_count, o.len.ptr(), e.remove_low,
                       o.b_out.as<double>(), o.b_scal.as<double>());
    TRY(o.close(false));
    return first_for_present(e);
}
