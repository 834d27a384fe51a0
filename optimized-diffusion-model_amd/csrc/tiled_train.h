// Training step on the TILED plan (fp32; shapes beyond one workgroup per sample, e.g. the CIFAR-shape model of BASELINE config #5).
// Included by rdmi.hip after train_plan.h; rdmi_enable_training / rdmi_train_forward / rdmi_backward branch here on c->tiled.
//
// Forward: the ordinary tiled forward (run_tiled), handed the step's dropout probability and seed word (FwdIn::drop_p / seed_dev): the
// launch loop applies Dropout_0 in the GroupNorm+SiLU staging of the convs flagged TConvL::dropout (every res block's Conv_1; Philox
// mask of (step seed in device memory, launch index, source element)).  The plan itself is not written to.  The tiled workspace is
// never reused (TiledBuilder::talloc only grows), so every tensor the backward needs -- layer inputs, GroupNorm statistics, softmax
// probabilities -- is still in place afterwards.
// Backward: the launch list in reverse into a gradient twin of the workspace (same offsets), zeroed once per step: every
// launch ADDS its input gradients into the twin, so a tensor read by several launches (skip tensors, the residual stream)
// collects their sum; the gradient of a conv's output is complete when its producer is reached.  Kernels: tiled_bwd_kernels.h.
// What the backward needs to know about a launch is on its record (csrc/tiled_plan.h), written when the plan was built: a TConvL
// carries the indices and layout of its weight / bias / GroupNorm parameters (TConvParams) and its dropout flag, the P V launch of
// an attention block carries the index of its Q K^T launch (TBgemmL::qk).  Launch names are not consulted.
#pragma once
#include "tiled_bwd_kernels.h"

namespace {

struct TiledTrain {
    dev_ptr<float> gws;                                // gradient twin of the tiled workspace (ws_per_sample * max_batch floats)
    dev_ptr<float> gfin;                               // NHWC gradient of the network output
    dev_ptr<float> act, dact, wslab, cs, gred, gslab;
    static constexpr int MAX_SPLIT = 16;               // weight-gradient K splits (slab depth)
    int last_B = 0; float drop_p = 0.f;
};

inline float* tl_gptr(rdmi_ctx* c, const TiledTrain& tt, size_t off) {
    if (off == T_NONE || off == T_XIN) return nullptr;
    return tt.gws.get() + off * (size_t)c->max_batch;
}

int tiled_enable_training(rdmi_ctx* c, TrainPlan& T) {
    if (c->arch.compute_dtype != 0) return fail("training on the tiled plan is built for fp32 only (train_dtype='bf16' on this shape is not built)");
    T.tiled = std::make_unique<TiledTrain>();
    TiledTrain* tt = T.tiled.get();
    const size_t NBmax = (size_t)c->max_batch;
    T.poff.resize(c->params.size());
    T.ptotal = 0;
    for (size_t i = 0; i < c->params.size(); ++i) { T.poff[i] = T.ptotal; T.ptotal += c->params[i].numel; }
    size_t act_f = 1, dact_f = 1, slab_f = 1; int cmax = 64;
    for (const TLaunch& tl : c->tiled->launches) {
        const TConvL* l = std::get_if<TConvL>(&tl.op);
        if (std::holds_alternative<TGnActL>(tl.op) || std::holds_alternative<TFlashL>(tl.op) || (l && l->pre)) return fail("tiled training: launch %s is a bf16-plan launch", tl.name.c_str());
        if (!l) continue;
        const TConvArgs& a = l->a;
        const int Cin = a.CA + a.CB;
        if (l->p_gamma >= 0) {
            if (a.up || a.stride != 1) return fail("tiled training: GroupNorm ahead of a resampling conv (%s)", tl.name.c_str());
            act_f = std::max(act_f, (size_t)a.Hv * a.Wv * Cin);
        }
        if (!l->in_is_x) dact_f = std::max(dact_f, (size_t)a.Hv * a.Wv * Cin);
        slab_f = std::max(slab_f, (size_t)a.ntap * a.Cout * Cin * TiledTrain::MAX_SPLIT);
        cmax = std::max(cmax, std::max(a.Cout, Cin));
    }
    const size_t E = (size_t)c->H * c->W * c->arch.channels, Mp = (size_t)pad16(c->max_batch);
    HIP_OK(hip_alloc(tt->gws, c->tiled->ws_per_sample * NBmax));
    HIP_OK(hip_alloc(tt->gfin, E * NBmax));
    HIP_OK(hip_alloc(tt->act, act_f * NBmax));
    HIP_OK(hip_alloc(tt->dact, dact_f * NBmax));
    HIP_OK(hip_alloc(tt->wslab, slab_f));
    HIP_OK(hip_alloc(tt->cs, (size_t)cmax * NBmax));
    HIP_OK(hip_alloc(tt->gslab, (size_t)cmax * 2 * NBmax));
    HIP_OK(hip_alloc(tt->gred, (size_t)32 * 2 * NBmax));
    // embedding backward (embed_backward) and step inputs
    HIP_OK(hip_alloc(T.gdense, Mp * c->dense_total));
    HIP_OK(hip_alloc(T.gta, Mp * c->temb));
    HIP_OK(hip_alloc(T.gh1, Mp * c->temb));
    HIP_OK(hip_alloc(T.four, Mp * 2 * c->arch.nf));
    T.emb_jobs = std::max(64, 2 * (c->dense_total / 32 + 1) + 8);   // two jobs per res block (>= 32 channels each) + the time / label stages
    HIP_OK(hip_alloc(T.d_gemm_jobs, (size_t)T.emb_jobs));
    HIP_OK(hip_alloc(T.d_col_jobs, (size_t)T.emb_jobs));
    T.h_gemm_jobs.reserve((size_t)T.emb_jobs); T.h_col_jobs.reserve((size_t)T.emb_jobs);
    HIP_OK(hip_alloc(T.sig_copy, Mp));
    HIP_OK(hip_alloc(T.lab_copy, Mp * std::max(1, c->arch.num_classes)));
    HIP_OK(hip_alloc(T.d_seed, 8));
    HIP_OK(hipMemset(T.d_seed.get(), 0, 64));
    HIP_OK(hip_alloc(T.h_seed, 64));
    T.use_graph = false;                               // plain launches on the caller's stream
    T.ready = true;
    return 0;
}

int tiled_train_forward(rdmi_ctx* c, TrainPlan& T, const float* x, const float* sigma, const float* labels, float* out, int B, float dropout_p,
                        uint64_t seed, hipStream_t s) {
    TiledTrain& tt = *T.tiled;
    if (int e = do_repack(c, s)) return e;
    HIP_OK(hipMemcpyAsync(T.sig_copy.get(), sigma, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (labels) HIP_OK(hipMemcpyAsync(T.lab_copy.get(), labels, (size_t)B * c->arch.num_classes * sizeof(float), hipMemcpyDeviceToDevice, s));
    T.seed_slot = (T.seed_slot + 1) & 63;
    T.h_seed.get()[T.seed_slot] = seed;
    HIP_OK(hipMemcpyAsync(T.d_seed.get(), T.h_seed.get() + T.seed_slot, sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    FwdIn f{x, 0, T.sig_copy.get(), 0, 0.f, 0, 0.f, 0.f, labels ? T.lab_copy.get() : nullptr, B, out, B};
    f.drop_p = dropout_p; f.seed_dev = T.d_seed.get();
    const int e = run_forward(c, f, s);
    if (c->profiling) prof_collect(c);
    tt.last_B = B; tt.drop_p = dropout_p; T.last_B = B;
    return e;
}

// backward of one conv launch: G (in place) -> bias / Dense_0 -> weight gradient -> data gradient -> GroupNorm / resampling adjoint.
// grads_flat == null (VJP-only): the launches that feed only parameter gradients are left out (bias / Dense_0 sums, the activation
// recompute and the weight-gradient contraction with its slab reduce, the gamma / beta row sums).  grad_x != null: the input conv's
// data gradient goes straight to the caller's NCHW grad_x (input_dgrad_kernel; no gradient twin of the input exists).
int tiled_conv_backward(rdmi_ctx* c, TrainPlan& T, TiledTrain& tt, const TConvL& l, int li, float* grads_flat, float* grad_x, int NB, hipStream_t s) {
    const TConvArgs& a = l.a; const TConvParams& b = l.w;
    const int Cin = a.CA + a.CB, HWo = a.Ho * a.Wo, HWv = a.Hv * a.Wv;
    const bool want_p = grads_flat != nullptr;
    auto pgrad = [&](int pi) -> float* { return pi >= 0 ? grads_flat + T.poff[(size_t)pi] : nullptr; };
    float* G = l.out_is_final ? tt.gfin.get() : tl_gptr(c, tt, l.oOut);
    {   // G = out_scale / sigma_n * dY (in place); residual gradient; column sums
        const float* sig = (l.out_is_final && c->arch.scale_by_sigma) ? T.sig_copy.get() : nullptr;
        ProfScope ps(c, s, "tb_outgrad_kernel", 0);
        hipLaunchKernelGGL(tb_outgrad_kernel, dim3((unsigned)ceil_div(a.Cout, 64), (unsigned)NB), dim3(RDMI_THREADS), 0, s, (const float*)G, G,
                           tl_gptr(c, tt, l.oResid), tt.cs.get(), HWo, a.Cout, a.out_scale, sig);
    }
    if (want_p) {
        ProfScope ps(c, s, "tb_bias_kernel", 0);
        hipLaunchKernelGGL(tb_bias_kernel, dim3((unsigned)ceil_div(a.Cout, RDMI_THREADS)), dim3(RDMI_THREADS), 0, s, (const float*)tt.cs.get(), NB, a.Cout,
                           pgrad(b.pb[0]), pgrad(b.pb[1]), pgrad(b.pb[2]), b.co_blk, l.use_dense ? T.gdense.get() : (float*)nullptr, c->dense_total, a.dense_off);
    }
    const bool gn = l.p_gamma >= 0;
    TbGnArgs g{};
    g.A = a.srcA; g.B = a.srcB; g.CA = a.CA; g.CB = a.CB; g.HW = a.Ha * a.Wa; g.NB = NB;
    g.stats = a.stats; g.G = a.G; g.Cg = a.Cg; g.act = a.act; g.gamma = a.gamma; g.beta = a.beta;
    g.drop_p = l.dropout ? tt.drop_p : 0.f; g.op_id = (uint32_t)li; g.seed_dev = T.d_seed.get();
    g.ACT = tt.act.get(); g.dACT = tt.dact.get(); g.red = tt.gred.get(); g.gslab = tt.gslab.get();
    g.gA = tl_gptr(c, tt, l.oA); g.gB = tl_gptr(c, tt, l.oB);
    g.up = a.up; g.Hv = a.Hv; g.Wv = a.Wv; g.has_gn = gn ? 1 : 0;
    if (gn && want_p) {   // the activated input, recomputed (GroupNorm + SiLU + the step's dropout mask): only the weight gradient reads it
        ProfScope ps(c, s, "tb_act_kernel", 0);
        hipLaunchKernelGGL(tb_act_kernel, grid1d((long)NB * HWv * Cin), dim3(RDMI_THREADS), 0, s, g);
    }
    if (want_p) {   // weight gradient: K = samples x output pixels split into <= MAX_SPLIT chunks, slab summed in a fixed order
        TbGemmArgs w{};
        w.M = a.Cout; w.N = Cin; w.K = NB * HWo;
        w.Hv = a.Hv; w.Wv = a.Wv; w.Ho = a.Ho; w.Wo = a.Wo; w.stride = a.stride; w.pad = a.pad_lo; w.ntap = a.ntap; w.Cin = Cin; w.Cout = a.Cout;
        w.G = G;
        if (gn) { w.X = tt.act.get(); w.X2 = nullptr; w.CA = Cin; w.CB = 0; w.Ha = a.Hv; w.Wa = a.Wv; w.up = 0; }
        else { w.X = a.srcA; w.X2 = a.srcB; w.CA = a.CA; w.CB = a.CB; w.Ha = a.Ha; w.Wa = a.Wa; w.up = a.up; }
        const long tiles = (long)ceil_div(a.Cout, 64) * ceil_div(Cin, 64) * a.ntap;
        int ns = (int)std::max(1L, std::min((long)TiledTrain::MAX_SPLIT, 1024 / tiles));
        ns = std::max(1, std::min(ns, ceil_div(w.K, 256)));
        w.kchunk = ceil_div(ceil_div(w.K, ns), 16) * 16; ns = ceil_div(w.K, w.kchunk); w.nsplit = ns;
        w.out = tt.wslab.get();
        {
            ProfScope ps(c, s, "tb_gemm_kernel<wgrad>", 2.0 * NB * HWo * a.ntap * (double)a.Cout * Cin);
            hipLaunchKernelGGL(tb_gemm_kernel<2>, dim3((unsigned)ceil_div(a.Cout, 64), (unsigned)ceil_div(Cin, 64), (unsigned)(a.ntap * ns)), dim3(RDMI_THREADS), 0, s, w);
        }
        ProfScope ps(c, s, "tb_wgrad_reduce_kernel", 0);
        hipLaunchKernelGGL(tb_wgrad_reduce_kernel, grid1d((long)a.ntap * a.Cout * Cin), dim3(RDMI_THREADS), 0, s, (const float*)tt.wslab.get(), ns, a.ntap,
                           a.Cout, Cin, pgrad(b.pw[0]), pgrad(b.pw[1]), pgrad(b.pw[2]), b.co_blk, b.w_co, b.w_ci, b.w_t);
    }
    if (l.in_is_x) return grad_x ? launch_input_dgrad(c, G, 0, grad_x, NB, s) : 0;   // the network input: only on request
    {   // data gradient over the virtual input grid
        TbGemmArgs d{};
        d.M = NB * HWv; d.N = Cin; d.K = a.ntap * a.Cout;
        d.Hv = a.Hv; d.Wv = a.Wv; d.Ho = a.Ho; d.Wo = a.Wo; d.stride = a.stride; d.pad = a.pad_lo; d.ntap = a.ntap; d.Cin = Cin; d.Cout = a.Cout;
        d.G = G;
        for (int i = 0; i < 3; ++i) d.W[i] = b.pw[i] >= 0 ? c->params[(size_t)b.pw[i]].ptr : nullptr;
        d.co_blk = b.co_blk; d.w_co = b.w_co; d.w_ci = b.w_ci; d.w_t = b.w_t;
        d.out = tt.dact.get();
        ProfScope ps(c, s, "tb_gemm_kernel<dgrad>", 2.0 * NB * HWo * a.ntap * (double)a.Cout * Cin);
        hipLaunchKernelGGL(tb_gemm_kernel<1>, dim3((unsigned)ceil_div(d.M, 64), (unsigned)ceil_div(Cin, 64), 1), dim3(RDMI_THREADS), 0, s, d);
    }
    if (gn) {
        {
            ProfScope ps(c, s, "tb_gn_red_kernel", 0);
            hipLaunchKernelGGL(tb_gn_red_kernel, dim3((unsigned)a.G, (unsigned)NB), dim3(RDMI_THREADS), 0, s, g);
        }
        if (want_p) {
            ProfScope ps(c, s, "tb_rowsum_kernel", 0);
            hipLaunchKernelGGL(tb_rowsum_kernel, dim3((unsigned)ceil_div(Cin, RDMI_THREADS)), dim3(RDMI_THREADS), 0, s, (const float*)tt.gslab.get(), NB, Cin, 2, 0, pgrad(l.p_gamma));
            hipLaunchKernelGGL(tb_rowsum_kernel, dim3((unsigned)ceil_div(Cin, RDMI_THREADS)), dim3(RDMI_THREADS), 0, s, (const float*)tt.gslab.get(), NB, Cin, 2, 1, pgrad(l.p_beta));
        }
    }
    ProfScope ps(c, s, "tb_src_grad_kernel", 0);
    hipLaunchKernelGGL(tb_src_grad_kernel, grid1d((long)NB * a.Ha * a.Wa * Cin), dim3(RDMI_THREADS), 0, s, g);
    return 0;
}

// AttnBlockpp core backward on the stored probabilities P (launch `pv`; q | k | v from launch `qk`):
//   dV = P^T dO, dP = dO V^T, dS = P o (dP - rowsum(dP o P)), dQ = alpha dS K, dK = alpha dS^T Q   (dP / dS live in the twin of S)
int tiled_attn_backward(rdmi_ctx* c, TiledTrain& tt, const TBgemmL& qk, const TBgemmL& pv, int NB, hipStream_t s) {
    // Lp: row stride of P and of its twin (L rounded up to whole K steps of the forward's P V; == L when L % 16 == 0).  Every contraction
    // here runs over L, and dP / dS are written over [L][L] only: the pad columns of the twin stay at the zeros of the step's memset and
    // never reach dQ or dK.
    const int L = pv.a.M, C = pv.a.N, Lp = pv.a.lda;
    const long C3 = 3L * C, LL = (long)L * Lp, LC3 = L * C3, LC = (long)L * C;
    const float* P = tl_ptr(c, pv.oA);
    const float* qkv = tl_ptr(c, qk.oA);
    float* dS = tl_gptr(c, tt, pv.oA);
    const float* dO = tl_gptr(c, tt, pv.oC);
    float* dqkv = tl_gptr(c, tt, qk.oA);
    const float alpha = qk.a.alpha;
    auto gemm = [&](int M, int N, int K, const float* A, long ab, long am, long ak, const float* B, long bb, long bk, long bn, float* Cp, long cb, long cm, long cn,
                    float al) {
        TbGemmArgs g{};
        g.M = M; g.N = N; g.K = K; g.A = A; g.a_b = ab; g.a_m = am; g.a_k = ak; g.B = B; g.b_b = bb; g.b_k = bk; g.b_n = bn;
        g.C = Cp; g.c_b = cb; g.c_m = cm; g.c_n = cn; g.alpha = al;
        ProfScope ps(c, s, "tb_gemm_kernel<attn>", 2.0 * M * N * K * NB);
        hipLaunchKernelGGL(tb_gemm_kernel<0>, dim3((unsigned)ceil_div(M, 64), (unsigned)ceil_div(N, 64), (unsigned)NB), dim3(RDMI_THREADS), 0, s, g);
    };
    gemm(L, C, L, P, LL, 1, Lp, dO, LC, C, 1, dqkv + 2 * C, LC3, C3, 1, 1.f);                // dV[j][c] = sum_i P[i][j] dO[i][c]
    gemm(L, L, C, dO, LC, C, 1, qkv + 2 * C, LC3, 1, C3, dS, LL, Lp, 1, 1.f);                // dP[i][j] = sum_c dO[i][c] V[j][c]
    {
        ProfScope ps(c, s, "tb_softmax_bwd_kernel", 0);
        hipLaunchKernelGGL(tb_softmax_bwd_kernel, dim3((unsigned)ceil_div(NB * L, 4)), dim3(RDMI_THREADS), 0, s, P, dS, (long)NB * L, L, Lp);
    }
    gemm(L, C, L, dS, LL, Lp, 1, qkv + C, LC3, C3, 1, dqkv, LC3, C3, 1, alpha);             // dQ[i][c] = alpha sum_j dS[i][j] K[j][c]
    gemm(L, C, L, dS, LL, 1, Lp, qkv, LC3, C3, 1, dqkv + C, LC3, C3, 1, alpha);             // dK[j][c] = alpha sum_i dS[i][j] Q[i][c]
    return 0;
}

int tiled_backward(rdmi_ctx* c, TrainPlan& T, const float* grad_out, float* grads_flat, size_t grads_numel, float* grad_x, hipStream_t s) {
    TiledTrain& tt = *T.tiled;
    if (grads_flat && grads_numel != T.ptotal) return fail("grads buffer holds %zu floats, the model has %zu parameters", grads_numel, T.ptotal);
    const int NB = tt.last_B;
    if (NB < 1) return fail("rdmi_backward before rdmi_train_forward");
    const size_t NBmax = (size_t)c->max_batch;
    const int HW = c->H * c->W, Cc = c->arch.channels;
    // every parameter gradient below is a store; time_embed.W (not trained) stays zero.  The twin takes sums: zeroed (all of it,
    // ws_per_sample * max_batch floats -- the tensors are [tensor][sample] blocks, so the first NB samples are not one range)
    if (grads_flat) HIP_OK(hipMemsetAsync(grads_flat, 0, T.ptotal * sizeof(float), s));
    HIP_OK(hipMemsetAsync(tt.gws.get(), 0, c->tiled->ws_per_sample * NBmax * sizeof(float), s));
    if (grads_flat) HIP_OK(hipMemsetAsync(T.gdense.get(), 0, (size_t)pad16(c->max_batch) * c->dense_total * sizeof(float), s));
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, grid1d((long)NB * HW * Cc), dim3(RDMI_THREADS), 0, s, grad_out, tt.gfin.get(), NB, HW, Cc, 0);
    const std::vector<TLaunch>& tl = c->tiled->launches;
    for (int li = (int)tl.size() - 1; li >= 0; --li) {
        if (const TConvL* l = std::get_if<TConvL>(&tl[(size_t)li].op)) {
            if (int e = tiled_conv_backward(c, T, tt, *l, li, grads_flat, grad_x, NB, s)) return e;
        } else if (const TBgemmL* pv = std::get_if<TBgemmL>(&tl[(size_t)li].op)) {
            if (pv->qk >= 0) { if (int e = tiled_attn_backward(c, tt, std::get<TBgemmL>(tl[(size_t)pv->qk].op), *pv, NB, s)) return e; }
        } else if (const TResizeL* l = std::get_if<TResizeL>(&tl[(size_t)li].op)) {   // nearest resize of h onto the skip grid: its twin is complete here (every reader comes later in the list)
            ResizeArgs ra = l->a; ra.NB = NB;
            ProfScope ps(c, s, "tb_resize_bwd_kernel", 0);
            hipLaunchKernelGGL(tb_resize_bwd_kernel, grid1d((long)NB * ra.Hs * ra.Ws * ra.C), dim3(RDMI_THREADS), 0, s, ra, (const float*)tl_gptr(c, tt, l->oDst),
                               tl_gptr(c, tt, l->oSrc));
        }
        // GroupNorm statistics (TStatsL / TStatsRecL): their gradient is part of the GroupNorm backward; softmax, transpose and Q K^T: inside the attention backward
        HIP_OK(hipGetLastError());
    }
    if (grads_flat) { if (int e = embed_backward(c, T, grads_flat, NB, s)) return e; }
    if (c->profiling) prof_collect(c);
    return 0;
}

}  // namespace
