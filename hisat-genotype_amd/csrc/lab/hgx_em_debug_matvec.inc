// Lab build only: the body of hgx_debug_matvec (one rows / cols pass with a chosen back-end; tools/time_matvec.py, tests/lab_cases.py).
    ARGCHK(cc && x_host && y_host && (which == 0 || which == 1) && backend >= 1 && backend <= 3);
    hgx_classes *c = const_cast<hgx_classes *>(cc);
    const int A = c->a_pad, C = c->n_classes;
    ARGCHK(C > 0);
    int rc = hgx_ensure_transposed(c, nullptr);
    if (rc) return rc;
    const int nx = which == 0 ? A : C, ny = which == 0 ? C : A;
    DevBuf b_x, b_y, b_pr, b_pr2, b_scal, b_q;
    ALLOC(b_x, (size_t)nx * 8); ALLOC(b_y, (size_t)ny * 8); ALLOC(b_pr, (size_t)std::max(nx, ny)); ALLOC(b_pr2, (size_t)std::max(nx, ny));
    ALLOC(b_scal, S_N * 8); ALLOC(b_q, (size_t)ny * 8);
    HIPCHK(hipMemcpy(b_x.p, x_host, (size_t)nx * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(b_pr.p, 1, (size_t)std::max(nx, ny)));
    HIPCHK(hipMemset(b_scal.p, 0, S_N * 8));
    std::vector<double> ones(ny, 1.0);
    HIPCHK(hipMemcpy(b_q.p, ones.data(), (size_t)ny * 8, hipMemcpyHostToDevice));
    double one = 1.0;
    HIPCHK(hipMemcpy(b_scal.as<double>() + S_TOT_A, &one, 8, hipMemcpyHostToDevice));
    MatVec m = which == 0 ? MatVec{c->d_bits, C, c->w64, A} : MatVec{c->d_bitsT, A, c->c64, C};
    if (backend == 2) { hgx_set_error("hgx_debug_matvec: back-end 2 (int8 MFMA) was measured slower twice and removed in round 6"); return HGX_EINVAL; }
    DevBuf b_M, b_part, b_cnt;
    if (backend == 3) {
        ALLOC(b_M, (size_t)m.n_words * m.n_rows * 8);
        hipLaunchKernelGGL(k_word_transpose, dim3((m.n_words + 31) / 32, (m.n_rows + 31) / 32), dim3(256), 0, nullptr, m.B, m.n_rows,
                           m.n_words, b_M.as<uint64_t>());
        ALLOC(b_part, (size_t)(m.n_words / 8) * m.n_rows * 8);
        ALLOC(b_cnt, (size_t)((m.n_rows + BLOCK - 1) / BLOCK) * 4);
        HIPCHK(hipMemset(b_cnt.p, 0, (size_t)((m.n_rows + BLOCK - 1) / BLOCK) * 4));
        m.M = b_M.as<uint64_t>(); m.n_pad = m.n_rows; m.part = b_part.as<double>(); m.counters = b_cnt.as<unsigned>();
    }
    const int saved = g_backend;
    g_backend = backend;
    const int reps = hgx_test_switch("dbg_reps") ? atoi(hgx_test_switch("dbg_reps")) : 1;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, nullptr);
    for (int rep = 0; rep < reps; ++rep)
    if (which == 0)
        rc = launch_matvec<MODE_ROWS>(m, nullptr, b_x.as<double>(), b_pr.as<uint8_t>(), 0, c->d_count, nullptr, nullptr, nullptr,
                                      b_y.as<double>(), nullptr, b_scal.as<double>(), 0);
    else   // q_in = 1, tot = 1, present everywhere: y = t
        rc = launch_matvec<MODE_COLS>(m, nullptr, b_x.as<double>(), nullptr, 0, nullptr, b_q.as<double>(), b_pr.as<uint8_t>(), nullptr,
                                      b_y.as<double>(), b_pr2.as<uint8_t>(), b_scal.as<double>(), 0);
    g_backend = saved;
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (reps > 1) fprintf(stderr, "[hgx_debug_matvec] which=%d backend=%d: %.2f us per launch\n", which, backend, ms * 1e3 / reps);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(y_host, b_y.p, (size_t)ny * 8, hipMemcpyDeviceToHost));
    return HGX_OK;
