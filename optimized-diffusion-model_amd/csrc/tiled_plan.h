// The TILED plan (kernels: csrc/tiled_kernels.h): NCSNpp.forward (RD/models/ncsnpp.py:226-354) as a list of launches over HBM-resident
// NHWC tensors, for shapes beyond one workgroup per sample (the CIFAR-shape model of BASELINE config #5).
// Included by rdmi.hip ahead of run_forward (build_plan, do_repack and run_forward call in here); tiled_train.h differentiates the list.
// A launch is one typed record (a std::variant: a kind without resolve_launch / run_launch below does not compile) holding its kernel's
// argument struct and the per-sample workspace offsets of its operands.  TiledBuilder fills it (build_tiled_plan), resolve_launch turns
// the offsets into pointers once the workspace exists (finish_tiled_plan), tiled_bind_params sets the parameter pointers at every
// repack, run_launch issues it (run_tiled).  A forward never writes to the plan.
#pragma once
#include <variant>

namespace {

// per-sample workspace offsets (floats) of the operands: T_NONE = absent, T_XIN = the NHWC copy of the caller's input
constexpr size_t T_NONE = (size_t)-1, T_XIN = (size_t)-2;

// a conv's parameters: where the packed weight sits in the arena, and which parameters it came from (the backward writes their gradients)
struct TConvParams {
    size_t w_off = 0; int job = -1, njob = 1;          // arena offset of the packed weight; its pack jobs (c->jobs[job .. job + njob))
    int pw[3] = {-1, -1, -1}, pb[3] = {-1, -1, -1};    // weight / bias parameter indices (q | k | v projection: three NIN matrices)
    int co_blk = 0; long w_co = 0, w_ci = 0, w_t = 0;  // parameter layout: OIHW (3x3) or NIN [in][out], co_blk output channels per matrix
    size_t bias_arena = T_NONE;                        // the bias is a packed arena row (q | k | v side by side) instead of parameter pb[0]
};

struct TConvL {                                        // tconv_kernel / tconv_pre_kernel / iconv_kernel
    TConvArgs a{};
    size_t oA = T_NONE, oB = T_NONE, oStats = T_NONE, oResid = T_NONE, oOut = T_NONE, oChsum = T_NONE;
    TConvParams w; int p_gamma = -1, p_beta = -1;      // GroupNorm parameters of the one-kernel form (-1: none, or applied by the TGnActL ahead)
    int nmt = 4; bool use_dense = false, in_is_x = false, out_is_final = false;   // nmt: 16-row tiles per wave (1: the output tile has 16 pixels or fewer)
    bool pre = false;                                  // the input is the bf16 tensor a TGnActL wrote, or the fused attention core's output (tconv_pre_kernel)
    bool dropout = false;                              // Conv_1 of a res block: the training forward applies Dropout_0 to its activated input
};
struct TStatsL { size_t oA = T_NONE, oB = T_NONE, oStats = T_NONE; const float *A = nullptr, *B = nullptr; float* stats = nullptr; int CA = 0, CB = 0, HW = 0, G = 0; };   // gn_stats_kernel: GroupNorm statistics by a pass over the tensor(s)
struct TStatsRecL {                                    // gn_finalize_kernel: statistics from the channel records the producing convs left (tiles / px: record count and pixels per full tile of each producer)
    size_t oCsA = T_NONE, oCsB = T_NONE, oStats = T_NONE; const float *csA = nullptr, *csB = nullptr; float* stats = nullptr; int CA = 0, CB = 0, tilesA = 0, tilesB = 0, pxA = 0, pxB = 0, HW = 0, G = 0;
};
struct TGnActL {                                       // gn_act_kernel / gn_act_fin_kernel: GroupNorm(+SiLU) written once as bf16 for a pre-activated conv
    GnActArgs a{}; int p_gamma = -1, p_beta = -1;
    size_t oA = T_NONE, oB = T_NONE, oStats = T_NONE, oOut = T_NONE, oOut2 = T_NONE, oCsA = T_NONE, oCsB = T_NONE;   // oOut2: raw bf16 copy of the input
    bool fin = false;                                  // statistics from the producers' channel records inside the launch (the TStatsRecL is folded in)
};
struct TBgemmL {                                       // bgemm_nt_kernel / bgemm_nt_bf16_kernel
    BgemmArgs a{}; size_t oA = T_NONE, oB = T_NONE, oC = T_NONE; long dB = 0;     // dB: B starts this many floats into its tensor (k inside q | k | v)
    int qk = -1;                                       // P V of an attention block: index of the block's Q K^T launch (-1: this is not P V)
};
struct TSoftmaxL { size_t oS = T_NONE; float* S = nullptr; long rows_per_sample = 0; int L = 0, Lp = 0; };   // softmax_rows_kernel (Lp: row stride, L rounded up to whole K steps of P V)
struct TTransposeL { size_t oSrc = T_NONE, oDst = T_NONE; const float* src = nullptr; float* dst = nullptr; int L = 0, C = 0, ld = 0, c0 = 0, Lp = 0; bool bf = false; };   // transpose_lc*_kernel: V^T [C][Lp] out of q | k | v (bf: bf16 elements; Lp: row stride of the output)
struct TFlashL { FlashArgs a{}; size_t oQkv = T_NONE, oVt = T_NONE, oOut = T_NONE; int C = 0; };   // flash_attn_bf16_kernel: fused softmax(Q K^T) V (bf16 plan)
struct TResizeL { ResizeArgs a{}; size_t oSrc = T_NONE, oDst = T_NONE; };                           // nearest_resize_kernel: h onto the skip tensor's grid (odd level grids)

struct TLaunch {
    std::string name; double flops_per_sample = 0;
    std::variant<TConvL, TStatsL, TStatsRecL, TGnActL, TBgemmL, TSoftmaxL, TTransposeL, TFlashL, TResizeL> op;
};

struct TiledPlan {
    std::vector<TLaunch> launches;
    dev_ptr<float> ws, xin, out; size_t ws_per_sample = 0;
    dev_ptr<unsigned char> zero;                       // 256 zero bytes: iconv_kernel's source for window pixels outside the image
    long min_wgs = 512;                                // a tiled conv widens its workgroups (NCT column tiles per wave) while the launch keeps this many (RDMI_TILED_MIN_WGS: tests)
    long iconv_min_wgs = LONG_MAX;                     // iconv_kernel from this many 128 x 128 tiles per launch (off unless RDMI_ICONV=1 / RDMI_ICONV_MIN_WGS)
};

struct TiledBuilder {
    rdmi_ctx* c; Builder& b; TiledPlan& p;
    size_t top = 0;                                   // floats per sample allocated so far
    struct TT { size_t off = 0; int C = 0, H = 0, W = 0; bool valid = false; size_t cs = T_NONE; int tiles = 0, tile_px = 0; bool bf = false; bool raw16 = false; int launch = -1; };   // raw16: q | k | v stored as bf16 [HW][3C]: only the fused attention core and its V transpose read it   // cs: per-tile channel sums of the producer; bf: a bf16 [HW][C] tensor (C % 64 == 0) for tconv_pre   // launch: a statistics tensor: index of the launch that writes it
    TT talloc(int C, int H, int W) { TT t; t.off = top; t.C = C; t.H = H; t.W = W; t.valid = true; top += ((size_t)C * H * W + 63) & ~(size_t)63; return t; }
    static int pad32(int a) { return (a + 31) & ~31; }
    template <class R> void push(const std::string& name, double flops_per_sample, const R& r) { p.launches.push_back({name, flops_per_sample, r}); }

    bool bf16() const { return c->arch.compute_dtype == 1; }
    // the weight of a 3x3 conv (`pre`.weight, OIHW) or a 1x1 conv (`pre`.W, NIN [in][out]) packed as fp32 [tap][K/16][Np][16], or as the
    // bf16 copy [tap][K/32][Np][32] (half the arena floats)
    TConvParams pack(const std::string& pre, int ntap, int cin, int cout) {
        const int Kp = pad32(cin), Np = pad16(cout);
        const bool nin = ntap == 1;
        TConvParams w; w.co_blk = cout; w.w_co = nin ? 1 : (long)cin * 9; w.w_ci = nin ? cout : 9; w.w_t = nin ? 0 : 1;
        w.w_off = b.alloc_w(bf16() ? ((size_t)ntap * Kp * Np + 1) / 2 : (size_t)ntap * Kp * Np); w.job = (int)c->jobs.size();
        b.job_pack(pre + (nin ? ".W" : ".weight"), w.w_off, cin, cout, Kp, Np, 0, ntap, w.w_co, w.w_ci, w.w_t);
        if (bf16()) c->jobs.back().kind = 2;
        w.pw[0] = c->pindex.at(pre + (nin ? ".W" : ".weight")); w.pb[0] = c->pindex.at(pre + (nin ? ".b" : ".bias"));
        return w;
    }
    TT stats(const std::string& name, const TT& A, const TT* B) {
        const int C = A.C + (B ? B->C : 0), G = std::min(C / 4, 32);
        TT st = talloc(2 * G, 1, 1);
        st.launch = (int)p.launches.size();
        if (A.cs != T_NONE && (!B || B->cs != T_NONE) && std::getenv("RDMI_TILED_STATS_PASS") == nullptr) {
            // statistics from the channel sums the producing convs left behind: no pass over the tensors
            TStatsRecL f; f.oCsA = A.cs; f.oCsB = B ? B->cs : T_NONE; f.oStats = st.off; f.CA = A.C; f.CB = B ? B->C : 0; f.HW = A.H * A.W; f.G = G;
            f.tilesA = A.tiles; f.tilesB = B ? B->tiles : 0; f.pxA = A.tile_px; f.pxB = B ? B->tile_px : 0;
            push(name + ".stats", 0, f);
            return st;
        }
        TStatsL l; l.oA = A.off; l.oB = B ? B->off : T_NONE; l.oStats = st.off; l.CA = A.C; l.CB = B ? B->C : 0; l.HW = A.H * A.W; l.G = G;
        push(name + ".stats", 0, l);
        return st;
    }
    // conv over concat(A, B) [optionally GroupNorm(+SiLU)'d with `st`], 3x3 (stride 1 pad 1 | stride 2 Downsample | nearest x2 Upsample) or 1x1
    struct Spec {
        std::string name; const TT* A = nullptr; const TT* B = nullptr;   // the conv reads concat(A, B)
        const TT* st = nullptr; std::string gn; bool act = false;         // GroupNorm ahead of the conv: its statistics, parameter prefix, SiLU
        int ntap = 9, stride = 1; bool up = false; TConvParams w; int cout = 0;
        int dense_off = -1;                            // >= 0: the epilogue adds this column slice of Dense_0(SiLU(temb))
        const TT* resid = nullptr; float scale = 1.f;  // out = scale * (conv + resid)
        bool final_out = false, in_is_x = false, dropout = false, out16 = false;   // out16: the output is stored as bf16 (TT::raw16)
        TT* raw_copy = nullptr;                        // if the conv takes the pre-activated form, its activation pass also leaves the RAW input as a bf16 [HW][Cv] tensor here
    };
    TT conv(const Spec& q) {
        const TT &A = *q.A; const TT *B = q.B, *st = q.st; const int ntap = q.ntap, cout = q.cout;
        // bf16 plan: a 3x3 stride-1 conv behind a GroupNorm reads a tensor that was normalised, activated and rounded to bf16 ONCE
        // (TGnActL) instead of redoing that arithmetic for every staged window element (RDMI_NO_PREACT=1: the one-kernel form)
        // (3x3 stride-1 convs and the 1x1 q/k/v projection of attention blocks); a tensor that already is bf16 (the fused attention
        // core's output) goes to the same kernel without the extra pass.
        const bool direct = A.bf && !B && !st && ntap == 1;
        const bool pre = direct || (bf16() && st && (ntap == 9 || ntap == 1) && q.stride == 1 && !q.up && !q.final_out && cout % 16 == 0 && A.C % 4 == 0 &&
                                    (!B || B->C % 4 == 0) && (A.C + (B ? B->C : 0)) % 64 == 0 && std::getenv("RDMI_NO_PREACT") == nullptr);
        if (A.bf && !direct) throw std::runtime_error("tiled plan: a bf16 tensor feeds a conv that cannot take it (" + q.name + ")");
        if (A.raw16 || (B && B->raw16) || (q.resid && q.resid->raw16)) throw std::runtime_error("tiled plan: a bf16-stored q | k | v tensor is read by a conv (" + q.name + ")");
        size_t act_off = A.off;
        if (pre && !direct) {
            const int Cin = A.C + (B ? B->C : 0), Cvp = pad32(Cin);
            TT actT = talloc((Cvp + 1) / 2, A.H, A.W);               // bf16 [HW][Cv]
            act_off = actT.off;
            TGnActL g; g.oA = A.off; g.oB = B ? B->off : T_NONE; g.oStats = st->off; g.oOut = actT.off;
            if (q.raw_copy && std::getenv("RDMI_NO_RAW_COPY") == nullptr) {
                *q.raw_copy = talloc((Cvp + 1) / 2, A.H, A.W);
                q.raw_copy->C = Cvp; q.raw_copy->bf = true;
                g.oOut2 = q.raw_copy->off;
            }
            g.a.CA = A.C; g.a.CB = B ? B->C : 0; g.a.Cv = Cvp; g.a.HW = A.H * A.W;
            g.a.G = std::min(Cin / 4, 32); g.a.Cg = Cin / g.a.G; g.a.act = q.act ? 1 : 0;
            g.p_gamma = c->pindex.at(q.gn + ".weight"); g.p_beta = c->pindex.at(q.gn + ".bias");
            // the statistics launch of this GroupNorm (a TStatsRecL: from the producers' channel records) is folded into the activation pass:
            // gn_act_fin_kernel reads the records itself (RDMI_NO_GN_FOLD=1 keeps the two launches)
            int max_slots = 0;                                          // groups a 64-channel slice touches (the kernel's table holds 16)
            for (int c_lo = 0; c_lo < Cin; c_lo += 64) max_slots = std::max(max_slots, (std::min(c_lo + 64, Cin) - 1) / g.a.Cg - c_lo / g.a.Cg + 1);
            const TStatsRecL* f = std::get_if<TStatsRecL>(&p.launches[(size_t)st->launch].op);
            if (f && Cvp % 64 == 0 && max_slots <= 16 && g.a.Cg <= 16 && std::getenv("RDMI_NO_GN_FOLD") == nullptr) {
                g.fin = true; g.oCsA = f->oCsA; g.oCsB = f->oCsB;
                g.a.tilesA = f->tilesA; g.a.tilesB = f->tilesB; g.a.pxA = f->pxA; g.a.pxB = f->pxB; g.a.eps = 1e-6f;
                p.launches.erase(p.launches.begin() + st->launch);
            }
            push(q.name + ".act", 0, g);
        }
        TConvL l; l.w = q.w;
        TConvArgs& a = l.a;
        a.CA = A.C; a.CB = B ? B->C : 0; a.Cv = pad32(a.CA + a.CB);
        if (pre) { a.CA = a.Cv; a.CB = 0; }
        a.Ha = A.H; a.Wa = A.W; a.up = q.up ? 1 : 0; a.Hv = q.up ? 2 * A.H : A.H; a.Wv = q.up ? 2 * A.W : A.W;
        a.stride = q.stride; a.ntap = ntap; a.pad_lo = (ntap == 9 && q.stride == 1) ? 1 : 0;
        a.Ho = q.stride == 2 ? (a.Hv + 1 - 3) / 2 + 1 : a.Hv; a.Wo = q.stride == 2 ? (a.Wv + 1 - 3) / 2 + 1 : a.Wv;
        a.TR = a.Wo >= 64 ? 1 : std::max(1, std::min(a.Ho, 64 / a.Wo));
        if (st && !pre) { a.G = std::min((a.CA + a.CB) / 4, 32); a.Cg = (a.CA + a.CB) / a.G; a.act = q.act ? 1 : 0; }
        a.dense_off = q.dense_off < 0 ? 0 : q.dense_off; a.dense_stride = c->dense_total;
        a.out_scale = q.scale;
        a.Cout = cout; a.Cout_pad = pad16(cout);
        // bf16 packs: interleave the weights' columns by the NCT the launch will use at the sampling batch (run_launch's rule at 128 forwards),
        // so that the epilogue's loads and stores are 8- / 16-byte vectors over full lines (tconv_epilogue; RDMI_NO_COL_IL=1: plain order)
        if (bf16() && std::getenv("RDMI_NO_COL_IL") == nullptr) {
            const long tl = ceil_div(a.Ho, a.TR);
            for (int cand : {4, 2})
                if (cout % (16 * cand) == 0 && a.Cout_pad >= 64 * cand && tl * 128 * ceil_div(a.Cout_pad, 64 * cand) >= 512) { a.col_il = cand; break; }
            for (int j = 0; a.col_il > 1 && j < q.w.njob; ++j) c->jobs[(size_t)(q.w.job + j)].col_il = a.col_il;
        }
        TT out = talloc(q.out16 ? (cout + 1) / 2 : cout, a.Ho, a.Wo);
        out.C = cout; out.raw16 = q.out16; a.out_bf16 = q.out16 ? 1 : 0;
        if (!q.final_out && cout % 4 == 0) {
            out.tiles = ceil_div(a.Ho, a.TR); out.tile_px = a.TR * a.Wo;
            TT cs = talloc(2 * cout * out.tiles, 1, 1);
            out.cs = l.oChsum = cs.off;
        }
        l.oA = A.off; l.oB = B ? B->off : T_NONE; l.oStats = st ? st->off : T_NONE;
        if (pre) { l.pre = true; l.oA = act_off; l.oB = T_NONE; l.oStats = T_NONE; }
        l.oResid = q.resid ? q.resid->off : T_NONE; l.oOut = out.off;
        l.nmt = (a.TR * a.Wo > 16) ? 4 : 1;
        if (st && !pre) { l.p_gamma = c->pindex.at(q.gn + ".weight"); l.p_beta = c->pindex.at(q.gn + ".bias"); }
        l.in_is_x = q.in_is_x; l.out_is_final = q.final_out; l.dropout = q.dropout; l.use_dense = q.dense_off >= 0;
        push(q.name, 2.0 * a.Ho * a.Wo * cout * (double)ntap * (A.C + (B ? B->C : 0)), l);
        return out;
    }
    // the spec of conv `name` over A with its own parameters (`name`.weight / .bias, or .W / .b for 1x1), which are packed here
    Spec spec(const std::string& name, const TT& A, int ntap, int cin, int cout) { Spec q; q.name = name; q.A = &A; q.ntap = ntap; q.w = pack(name, ntap, cin, cout); q.cout = cout; return q; }
    TT resblock(const std::string& name, const TT& A, const TT* B, int cout, int dense_off) {
        const int cin = A.C + (B ? B->C : 0);
        TT st0 = stats(name + ".GroupNorm_0", A, B);
        // bf16 plan: GroupNorm_0's activation pass reads the block's raw input anyway and leaves a bf16 copy of it for the NIN_0
        // shortcut, which then is a copy-staged 1x1 conv over half the bytes instead of a conv that converts fp32 while staging
        TT xraw;
        Spec c0 = spec(name + ".Conv_0", A, 9, cin, cout);
        c0.B = B; c0.st = &st0; c0.gn = name + ".GroupNorm_0"; c0.act = true; c0.dense_off = dense_off; c0.raw_copy = cin != cout ? &xraw : nullptr;
        TT h1 = conv(c0);
        TT st1 = stats(name + ".GroupNorm_1", h1, nullptr);
        Spec c1 = spec(name + ".Conv_1", h1, 9, cout, cout);
        c1.st = &st1; c1.gn = name + ".GroupNorm_1"; c1.act = true; c1.scale = (float)(1.0 / std::sqrt(2.0)); c1.dropout = true; c1.resid = &A;
        TT sc;
        if (cin != cout) {
            Spec n = spec(name + ".NIN_0", xraw.valid ? xraw : A, 1, cin, cout); n.B = xraw.valid ? nullptr : B;
            sc = conv(n); c1.resid = &sc;
        }
        return conv(c1);
    }
    // h resized onto the skip tensor's grid (RD/models/ncsnpp.py:319-320; an odd level grid: 5x5 -> Downsample -> 2x2 -> Upsample -> 4x4):
    // the resized NHWC tensor is materialised, so everything downstream reads an ordinary tensor.  It carries no channel records (TT::cs
    // unset): the producer's records are sums over the SOURCE grid, and the pixel multiplicities differ after the resize, so the
    // GroupNorm over concat(resized, skip) takes the pass over the tensors (TStatsL).
    TT resize(const std::string& name, const TT& A, int Hd, int Wd) {
        if (A.bf || A.raw16 || A.C % 4 != 0) throw std::runtime_error("tiled plan: " + name + " needs an fp32 tensor with C % 4 == 0");
        TT out = talloc(A.C, Hd, Wd);
        TResizeL l; l.oSrc = A.off; l.oDst = out.off;
        l.a.Hs = A.H; l.a.Ws = A.W; l.a.Hd = Hd; l.a.Wd = Wd; l.a.C = A.C;
        l.a.sh = (float)A.H / Hd; l.a.sw = (float)A.W / Wd;
        push(name, 0, l);
        return out;
    }
    // AttnBlockpp (RD/models/layerspp.py:67-96): GN -> q,k,v (one 1x1 conv, Cout = 3C) -> softmax(q k^T / sqrt(C)) v -> NIN_3 -> (x + h)/sqrt2
    TT attn(const std::string& name, const TT& x) {
        const int C = x.C, Lq = x.H * x.W;
        // C % 32: the q | k | v pack is laid out with K = C unpadded while the 1x1 conv contracts pad32(C) channels.  Q K^T contracts K = C
        // and P V contracts K = L: bgemm_nt_kernel steps K by 16 and bgemm_nt_bf16_kernel by 32 (a last step of 16 is predicated), the row /
        // column tails of both are clamped and masked.  L % 16 != 0 (a 10x10 or 9x9 level): the rows of the score buffer and of V^T are
        // padded to Lp = L rounded up to 16 (bf16: 32, whole steps) and the pad is written as zeros by the softmax and the transpose, so P V
        // contracts K = Lp over aligned rows with the same result; L % 16 == 0 keeps Lp = L, the strides and launches it always had.
        // The fused bf16 core has its own rule below (C of 64 / 128 / 256 and L % 64 == 0) and every other bf16 shape takes the bgemm route.
        if (C % 32 != 0)
            throw std::runtime_error(name + ": tiled attention needs C % 32 == 0 (C = " + std::to_string(C) + ", H*W = " + std::to_string(Lq) + ")");
        const int Lp = Lq % 16 == 0 ? Lq : (bf16() ? (Lq + 31) & ~31 : (Lq + 15) & ~15);
        TT st = stats(name + ".GroupNorm_0", x, nullptr);
        TConvParams w3; w3.w_off = b.alloc_w(bf16() ? (size_t)3 * C * C / 2 : (size_t)3 * C * C);
        w3.co_blk = C; w3.w_co = 1; w3.w_ci = C; w3.w_t = 0; w3.job = (int)c->jobs.size(); w3.njob = 3;
        for (int i = 0; i < 3; ++i) {
            PackJob j{};
            j.dst = reinterpret_cast<float*>(w3.w_off);
            j.Cin = C; j.Cout = C; j.Kpad = C; j.Npad = 3 * C; j.n_off = i * C; j.ntap = 1; j.s_co = 1; j.s_ci = C; j.s_t = 0; j.kind = bf16() ? 2 : 0;
            c->jobs.push_back(j);
            w3.pw[i] = c->pindex.at(name + ".NIN_" + std::to_string(i) + ".W"); w3.pb[i] = c->pindex.at(name + ".NIN_" + std::to_string(i) + ".b");
            c->job_param.push_back(w3.pw[i]);
        }
        w3.bias_arena = b.alloc_w((size_t)3 * C);
        for (int i = 0; i < 3; ++i) b.job_copy(name + ".NIN_" + std::to_string(i) + ".b", w3.bias_arena, C, i * C);
        const bool flash = bf16() && (C == 64 || C == 128 || C == 256) && Lq % 64 == 0 && std::getenv("RDMI_NO_FLASH") == nullptr;
        // the fused core rounds q, k, v to bf16 before its MFMAs anyway: the projection stores them as bf16 (half the conv's writes, half the
        // core's and the transpose's reads; same bits into the MFMAs when 1 / sqrt(C) is a power of two, C = 64 / 256).  RDMI_NO_QKV16=1: fp32
        const bool qkv16 = flash && C % 2 == 0 && std::getenv("RDMI_NO_QKV16") == nullptr;
        Spec pq; pq.name = name + ".qkv"; pq.A = &x; pq.ntap = 1; pq.w = w3; pq.cout = 3 * C; pq.st = &st; pq.gn = name + ".GroupNorm_0"; pq.out16 = qkv16;
        TT qkv = conv(pq);
        TT Vt = talloc(qkv16 ? C / 2 : C, Lp, 1);    // [C][Lp]
        TT O = talloc(C, x.H, x.W);
        TTransposeL vt; vt.oSrc = qkv.off; vt.oDst = Vt.off; vt.L = Lq; vt.C = C; vt.ld = 3 * C; vt.c0 = 2 * C; vt.Lp = flash ? Lq : Lp; vt.bf = qkv16;
        if (flash) {
            // bf16 plan: scores, softmax and P V in one kernel (no [L][L] buffer); V^T still comes from the transpose launch
            O.bf = true;                             // written as bf16 [L][C] (half of the allocation): NIN_3 stages plain copies of it
            push(name + ".vT", 0, vt);
            TFlashL l; l.oQkv = qkv.off; l.oVt = Vt.off; l.oOut = O.off;
            l.a.L = Lq; l.a.alpha = 1.0f / std::sqrt((float)C); l.C = C; l.a.out_bf16 = 1; l.a.in_bf16 = qkv16 ? 1 : 0;
            push(name + ".core", 4.0 * Lq * Lq * C, l);
        } else {
            TT S = talloc(Lq, Lp, 1);                // [L][Lp] scores / probabilities
            TBgemmL qk; qk.oA = qkv.off; qk.oB = qkv.off; qk.dB = C; qk.oC = S.off;
            qk.a.sa = qk.a.sb = (long)Lq * 3 * C; qk.a.sc = (long)Lq * Lp; qk.a.lda = qk.a.ldb = 3 * C; qk.a.ldc = Lp;
            qk.a.M = Lq; qk.a.N = Lq; qk.a.K = C; qk.a.alpha = 1.0f / std::sqrt((float)C);
            const int qk_launch = (int)p.launches.size();
            push(name + ".qk", 2.0 * Lq * Lq * C, qk);
            TSoftmaxL sm; sm.oS = S.off; sm.rows_per_sample = Lq; sm.L = Lq; sm.Lp = Lp;
            push(name + ".softmax", 0, sm);
            push(name + ".vT", 0, vt);
            TBgemmL pv; pv.qk = qk_launch; pv.oA = S.off; pv.oB = Vt.off; pv.oC = O.off;
            pv.a.sa = (long)Lq * Lp; pv.a.sb = (long)C * Lp; pv.a.sc = (long)Lq * C; pv.a.lda = Lp; pv.a.ldb = Lp; pv.a.ldc = C;
            pv.a.M = Lq; pv.a.N = C; pv.a.K = Lp; pv.a.alpha = 1.f;
            push(name + ".pv", 2.0 * Lq * Lq * C, pv);
        }
        Spec n3 = spec(name + ".NIN_3", O, 1, C, C); n3.resid = &x; n3.scale = (float)(1.0 / std::sqrt(2.0));
        return conv(n3);
    }
};

int build_tiled_plan(rdmi_ctx* c, Builder& b, const Layout& L, std::map<std::string, int>& dense_off) {
    const rdmi_arch& a = c->arch;
    using TT = TiledBuilder::TT;
    auto plan = std::make_unique<TiledPlan>();
    TiledBuilder t{c, b, *plan};
    int H = c->H, W = c->W;
    TT xin = t.talloc(a.channels, H, W);               // NHWC copy of the caller's NCHW input
    xin.off = T_XIN;                                   // marker: resolved to TiledPlan::xin
    TiledBuilder::Spec ci = t.spec("input_conv", xin, 9, a.channels, a.nf); ci.in_is_x = true;
    TT h = t.conv(ci);
    std::vector<TT> hs{h};
    int d = 0;
    for (int i = 0; i < a.n_levels; ++i) {
        for (int j = 0; j < a.num_res_blocks; ++j, ++d) {
            const BlockSpec& bs = L.down[(size_t)d];
            h = t.resblock(bs.name, h, nullptr, bs.cout, dense_off[bs.name]);
            if (bs.attn) h = t.attn("down_attn." + std::to_string(d), h);
            hs.push_back(h);
        }
        hs.push_back(h);
        if (i != a.n_levels - 1) {
            const std::string nm = "downsample." + std::to_string(i) + ".Conv_0";
            TiledBuilder::Spec q = t.spec(nm, h, 9, h.C, h.C); q.stride = 2;
            h = t.conv(q);
        }
    }
    h = t.resblock("mid_block1", h, nullptr, L.mid_ch, dense_off["mid_block1"]);
    if (a.attn_levels >> (a.n_levels - 1) & 1) return fail("attention at the bottleneck resolution (mid_attn) is not built");
    h = t.resblock("mid_block2", h, nullptr, L.mid_ch, dense_off["mid_block2"]);
    int u = 0;
    for (int k = 0; k < a.n_levels; ++k) {
        for (int j = 0; j < a.num_res_blocks + 1; ++j, ++u) {
            const BlockSpec& bs = L.up[(size_t)u];
            TT sk = hs.back();
            hs.pop_back();
            if (sk.H != h.H || sk.W != h.W) h = t.resize("resize." + std::to_string(u), h, sk.H, sk.W);
            h = t.resblock(bs.name, h, &sk, bs.cout, dense_off[bs.name]);
            if (bs.attn) h = t.attn("up_attn." + std::to_string(u), h);
        }
        if (k != a.n_levels - 1) {
            const std::string nm = "upsample." + std::to_string(k) + ".Conv_0";
            TiledBuilder::Spec q = t.spec(nm, h, 9, h.C, h.C); q.up = true;
            h = t.conv(q);
        }
    }
    if (h.H != c->H || h.W != c->W) return fail("network output grid %dx%d != input %dx%d", h.H, h.W, c->H, c->W);
    TT st = t.stats("out_norm", h, nullptr);
    TiledBuilder::Spec co = t.spec("out_conv", h, 9, h.C, a.channels);
    co.st = &st; co.gn = "out_norm"; co.act = true; co.final_out = true;
    t.conv(co);
    plan->ws_per_sample = t.top;
    c->tiled = std::move(plan);
    return 0;
}

// resolve a per-sample workspace offset to a device pointer (tensors are [tensor][n][...]: the offset scales with max_batch)
inline float* tl_ptr(const rdmi_ctx* c, size_t off, long delta = 0) {
    if (off == T_NONE) return nullptr;
    if (off == T_XIN) return c->tiled->xin.get();
    return c->tiled->ws.get() + off * (size_t)c->max_batch + delta;
}

// ---- workspace offsets -> pointers, once per context (the conv also checks that its window fits the kernel's staging)
int resolve_launch(rdmi_ctx* c, const std::string& name, TConvL& l) {
    TConvArgs& a = l.a;
    a.srcA = tl_ptr(c, l.oA); a.srcB = tl_ptr(c, l.oB); a.stats = tl_ptr(c, l.oStats); a.resid = tl_ptr(c, l.oResid);
    a.out = l.out_is_final ? c->tiled->out.get() : tl_ptr(c, l.oOut);
    a.wpk = c->d_w.get() + l.w.w_off;
    a.dense = l.use_dense ? c->d_dense.get() : nullptr;
    a.chsum = tl_ptr(c, l.oChsum);
    a.zeros = c->tiled->zero.get();
    if (l.pre && tconv_trv(a) * tconv_wl(a) * (a.ntap == 1 ? TpCfg<1>::UPP : TpCfg<9>::UPP) > TC_MAXS * RDMI_THREADS)
        return fail("tiled conv %s: window of %d pixels exceeds the register staging", name.c_str(), tconv_trv(a) * tconv_wl(a));
    if (l.pre && tconv_pre_lds_bytes(a) > 160 * 1024) return fail("tiled conv %s: LDS window %zu B", name.c_str(), tconv_pre_lds_bytes(a));
    if (tconv_lds_bytes(a) > 160 * 1024) return fail("tiled conv %s: LDS window %zu B", name.c_str(), tconv_lds_bytes(a));
    if (tconv_trv(a) * tconv_wl(a) * 8 > TC_MAXS * RDMI_THREADS) return fail("tiled conv %s: window of %d pixels exceeds the register staging (%d float4 per work-item)", name.c_str(), tconv_trv(a) * tconv_wl(a), TC_MAXS);
    return 0;
}
int resolve_launch(rdmi_ctx* c, const std::string&, TStatsL& l) { l.A = tl_ptr(c, l.oA); l.B = tl_ptr(c, l.oB); l.stats = tl_ptr(c, l.oStats); return 0; }
int resolve_launch(rdmi_ctx* c, const std::string&, TStatsRecL& l) { l.csA = tl_ptr(c, l.oCsA); l.csB = tl_ptr(c, l.oCsB); l.stats = tl_ptr(c, l.oStats); return 0; }
int resolve_launch(rdmi_ctx* c, const std::string&, TGnActL& l) {
    l.a.A = tl_ptr(c, l.oA); l.a.B = tl_ptr(c, l.oB); l.a.stats = tl_ptr(c, l.oStats);
    l.a.out = reinterpret_cast<bf16_t*>(tl_ptr(c, l.oOut));
    l.a.out2 = reinterpret_cast<bf16_t*>(tl_ptr(c, l.oOut2));
    if (l.fin) { l.a.csA = tl_ptr(c, l.oCsA); l.a.csB = tl_ptr(c, l.oCsB); l.a.stats = nullptr; }
    return 0;
}
int resolve_launch(rdmi_ctx* c, const std::string&, TBgemmL& l) { l.a.A = tl_ptr(c, l.oA); l.a.B = tl_ptr(c, l.oB, l.dB); l.a.C = tl_ptr(c, l.oC); return 0; }
int resolve_launch(rdmi_ctx* c, const std::string&, TSoftmaxL& l) { l.S = tl_ptr(c, l.oS); return 0; }
int resolve_launch(rdmi_ctx* c, const std::string&, TTransposeL& l) { l.src = tl_ptr(c, l.oSrc); l.dst = tl_ptr(c, l.oDst); return 0; }
int resolve_launch(rdmi_ctx* c, const std::string&, TFlashL& l) { l.a.qkv = tl_ptr(c, l.oQkv); l.a.vt = tl_ptr(c, l.oVt); l.a.out = tl_ptr(c, l.oOut); return 0; }
int resolve_launch(rdmi_ctx* c, const std::string&, TResizeL& l) { l.a.src = tl_ptr(c, l.oSrc); l.a.dst = tl_ptr(c, l.oDst); return 0; }

int finish_tiled_plan(rdmi_ctx* c) {
    TiledPlan& p = *c->tiled;
    const size_t NBmax = (size_t)c->max_batch;
    const size_t E = (size_t)c->H * c->W * c->arch.channels;
    HIP_OK(hip_alloc(p.ws, p.ws_per_sample * NBmax));
    HIP_OK(hip_alloc(p.xin, E * NBmax));
    HIP_OK(hip_alloc(p.out, E * NBmax));
    HIP_OK(hip_alloc(p.zero, 256));
    HIP_OK(hipMemset(p.zero.get(), 0, 256));
    // measured on MI355X (rocprofv3 kernel trace, B = 64 with guidance): 5.28 ms for the 3x3 convs of the 32x32 / 16x16 levels against 4.88 ms
    // with tconv_pre_kernel -- the implicit-GEMM form is NOT the default; RDMI_ICONV=1 selects it (from RDMI_ICONV_MIN_WGS tiles, default 256)
    if (const char* e = std::getenv("RDMI_TILED_MIN_WGS")) p.min_wgs = std::atol(e);
    if (const char* e = std::getenv("RDMI_ICONV")) if (std::atoi(e) != 0) p.iconv_min_wgs = 256;
    if (const char* e = std::getenv("RDMI_ICONV_MIN_WGS")) p.iconv_min_wgs = std::atol(e);
    for (auto& l : p.launches)
        if (int e = std::visit([&](auto& r) { return resolve_launch(c, l.name, r); }, l.op)) return e;
    return 0;
}

// ---- parameter pointers, at every repack: only the kinds that read parameters
void tiled_bind_params(rdmi_ctx* c) {
    auto P = [&](int pi) -> const float* { return pi < 0 ? nullptr : c->params[(size_t)pi].ptr; };
    for (auto& l : c->tiled->launches) {
        if (TConvL* r = std::get_if<TConvL>(&l.op)) { r->a.bias = r->w.bias_arena != T_NONE ? c->d_w.get() + r->w.bias_arena : P(r->w.pb[0]); r->a.gamma = P(r->p_gamma); r->a.beta = P(r->p_beta); }
        else if (TGnActL* g = std::get_if<TGnActL>(&l.op)) { g->a.gamma = P(g->p_gamma); g->a.beta = P(g->p_beta); }
    }
}

// ---- the launch loop
struct TRun {                                          // what one forward hands every launch
    rdmi_ctx* c; const FwdIn& f; hipStream_t s;
    const TLaunch* l = nullptr; int li = 0;            // the launch being issued, its index in the list (keys the dropout mask)
    // one kernel (256 work-items per workgroup) under the profile row `label`, credited with the launch's FLOPs
    template <class... KA, class... A> void launch(const std::string& label, void (*k)(KA...), dim3 grid, size_t lds, const A&... a) const {
        ProfScope ps(c, s, label, l->flops_per_sample * f.NB);
        hipLaunchKernelGGL(k, grid, dim3(RDMI_THREADS), lds, s, a...);
    }
};
inline dim3 grid1d(long n) { return dim3((unsigned)((n + RDMI_THREADS - 1) / RDMI_THREADS)); }

// the kernel of a conv launch: the instantiation for its tile shape (nmt 4 | 1 row tiles, nct 4 | 2 | 1 column tiles per wave) and its form
using TConvKernel = void (*)(TConvArgs);
template <int NMT, int NCT> TConvKernel tconv_form(bool pre, int ntap, bool h, bool drop) {
    if (pre) return ntap == 1 ? tconv_pre_kernel<NMT, NCT, 1> : tconv_pre_kernel<NMT, NCT, 9>;
    return h ? tconv_kernel<NMT, NCT, true> : drop ? tconv_kernel<NMT, NCT, false, true> : tconv_kernel<NMT, NCT, false>;
}
template <int NMT> TConvKernel tconv_cols(int nct, bool pre, int ntap, bool h, bool drop) {
    return nct == 4 ? tconv_form<NMT, 4>(pre, ntap, h, drop) : nct == 2 ? tconv_form<NMT, 2>(pre, ntap, h, drop) : tconv_form<NMT, 1>(pre, ntap, h, drop);
}

int run_launch(const TRun& R, const TConvL& l) {
    const rdmi_arch& arch = R.c->arch; const FwdIn& f = R.f; const int NB = f.NB;
    TConvArgs ca = l.a;
    ca.NB = NB;
    if (ca.dense && f.dense_rows) ca.dense = f.dense_rows;      // the sampler's per-update Dense_0 rows
    if (l.dropout && f.seed_dev) { ca.drop_p = f.drop_p; ca.op_id = (uint32_t)R.li; ca.seed_dev = f.seed_dev; }   // training forward: Dropout_0 (Philox mask of seed, launch index, element)
    if (l.out_is_final && arch.scale_by_sigma) {                // h / time_cond (RD/models/ncsnpp.py:350-351)
        if (f.sig) { ca.sig = f.sig; ca.sig_mod = f.sig_mod; ca.sig_is_time = f.t_is_time; ca.smin = f.smin; ca.ratio = f.ratio; }
        else ca.out_scale /= f.t_is_time ? f.smin * powf(f.ratio, f.t_scalar) : f.t_scalar;
    }
    const unsigned tiles = (unsigned)ceil_div(ca.Ho, ca.TR);
    // column tiles per wave (the workgroup covers 64 * nct channels: staging and its GroupNorm/SiLU arithmetic are shared), as
    // long as the launch still has >= 2 workgroups per CU
    int nct = 1;
    for (int cand : {4, 2})
        if (ca.Cout_pad >= 64 * cand && (long)tiles * NB * ceil_div(ca.Cout_pad, 64 * cand) >= R.c->tiled->min_wgs) { nct = cand; break; }
    const dim3 grid(tiles * (unsigned)NB, (unsigned)ceil_div(ca.Cout_pad, 64 * nct));
    const bool h = arch.compute_dtype == 1;
    const size_t lds = l.pre ? tconv_pre_lds_bytes(ca) : h ? tconv_bf16_lds_bytes(ca) : tconv_lds_bytes(ca);
    // implicit-GEMM form (iconv_kernel: 128 x 128 tiles over the whole batch's pixels) once the launch has a workgroup per CU
    // (read at context creation -- off by default, see finish_tiled_plan; RDMI_ICONV_MIN_WGS: tests set the threshold to reach the kernel at fixture batches)
    if (l.pre && ca.stride == 1 && !ca.up && ca.TR * ca.Wo == 64 && (ca.Ho * ca.Wo) % 64 == 0 && ca.Cout % 128 == 0 && ca.Cv % 64 == 0) {
        const long M = (long)NB * ca.Ho * ca.Wo;
        const dim3 g2((unsigned)((M + 127) / 128), (unsigned)(ca.Cout / 128));
        if ((long)g2.x * g2.y >= R.c->tiled->iconv_min_wgs) {
            static const bool by_shape = std::getenv("RDMI_PROF_SHAPES") != nullptr;      // diagnostic: one profile row per conv shape
            R.launch(by_shape ? "iconv_kernel<bf16> " + std::to_string(ca.Wo) + "x" + std::to_string(ca.Ho) + " K" + std::to_string(ca.ntap * ca.Cv) + " N" + std::to_string(ca.Cout) + (ca.resid ? " +res" : "") : std::string("iconv_kernel<bf16>"),
                     ca.ntap == 1 ? iconv_kernel<1> : iconv_kernel<9>, g2, iconv_lds_bytes(), ca);
            return 0;
        }
    }
    const bool drop = ca.drop_p > 0.f;
    R.launch(l.pre ? "tconv_pre_kernel<bf16>" : h ? "tconv_kernel<bf16>" : "tconv_kernel<fp32>",
             l.nmt == 4 ? tconv_cols<4>(nct, l.pre, ca.ntap, h, drop) : tconv_cols<1>(nct, l.pre, ca.ntap, h, drop), grid, lds, ca);
    return 0;
}
int run_launch(const TRun& R, const TStatsL& l) { R.launch("gn_stats_kernel", gn_stats_kernel, dim3((unsigned)l.G, (unsigned)R.f.NB), 16, l.A, l.B, l.CA, l.CB, l.HW, l.G, 1e-6f, l.stats); return 0; }
int run_launch(const TRun& R, const TStatsRecL& l) { R.launch("gn_finalize_kernel", gn_finalize_kernel, dim3((unsigned)R.f.NB), 0, l.csA, l.csB, l.CA, l.CB, l.tilesA, l.tilesB, l.pxA, l.pxB, l.HW, l.G, 1e-6f, l.stats); return 0; }
int run_launch(const TRun& R, const TGnActL& l) {
    GnActArgs g = l.a; g.NB = R.f.NB;
    if (l.fin) R.launch("gn_act_fin_kernel", gn_act_fin_kernel, dim3((unsigned)ceil_div(g.HW, GA_PIX), (unsigned)(g.Cv / 64), (unsigned)g.NB), gn_act_fin_lds_bytes(std::max(g.tilesA, g.tilesB)), g);
    else R.launch("gn_act_kernel", gn_act_kernel, grid1d((long)g.NB * g.HW * (g.Cv / 8)), 0, g);
    return 0;
}
int run_launch(const TRun& R, const TBgemmL& l) {
    const bool h = R.c->arch.compute_dtype == 1;
    R.launch(h ? "bgemm_nt_bf16_kernel" : "bgemm_nt_kernel", h ? bgemm_nt_bf16_kernel : bgemm_nt_kernel, dim3((unsigned)ceil_div(l.a.M, 64), (unsigned)ceil_div(l.a.N, 64), (unsigned)R.f.NB), 0, l.a);
    return 0;
}
int run_launch(const TRun& R, const TSoftmaxL& l) { const long rows = l.rows_per_sample * R.f.NB; R.launch("softmax_rows_kernel", softmax_rows_kernel, dim3((unsigned)((rows + 3) / 4)), 0, l.S, rows, l.L, l.Lp); return 0; }
int run_launch(const TRun& R, const TTransposeL& l) {
    const int NB = R.f.NB;
    const bool tile = l.L % 64 == 0 && l.C % 64 == 0;
    const dim3 tgrid((unsigned)(l.L / 64), (unsigned)(l.C / 64), (unsigned)NB);
    if (l.bf && !tile) return fail("bf16 q | k | v: the transpose needs L and C in multiples of 64");
    if (l.bf) R.launch("transpose_lc_kernel", transpose_lc_tile16_kernel, tgrid, 0, reinterpret_cast<const bf16_t*>(l.src), reinterpret_cast<bf16_t*>(l.dst), l.L, l.C, l.ld, l.c0);
    else if (tile) R.launch("transpose_lc_kernel", transpose_lc_tile_kernel, tgrid, 0, l.src, l.dst, l.L, l.C, l.ld, l.c0);
    else R.launch("transpose_lc_kernel", transpose_lc_kernel, grid1d((long)NB * l.Lp * l.C), 0, l.src, l.dst, NB, l.L, l.C, l.ld, l.c0, l.Lp);
    return 0;
}
int run_launch(const TRun& R, const TFlashL& l) {
    FlashArgs fa = l.a; fa.NB = R.f.NB;
    const dim3 grid((unsigned)(fa.L / 64), (unsigned)fa.NB);
    static bool flash_attr = false;                          // 70 KB of dynamic LDS at C = 256
    if (!flash_attr) {
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(flash_attn_bf16_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(flash_attn_bf16_kernel<128>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        flash_attr = true;
    }
    if (l.C == 256) R.launch("flash_attn_bf16_kernel", flash_attn_bf16_kernel<256>, grid, flash_lds_bytes<256>(), fa);
    else if (l.C == 128) R.launch("flash_attn_bf16_kernel", flash_attn_bf16_kernel<128>, grid, flash_lds_bytes<128>(), fa);
    else R.launch("flash_attn_bf16_kernel", flash_attn_bf16_kernel<64>, grid, flash_lds_bytes<64>(), fa);
    return 0;
}
int run_launch(const TRun& R, const TResizeL& l) {
    ResizeArgs ra = l.a; ra.NB = R.f.NB;
    R.launch("nearest_resize_kernel", nearest_resize_kernel, grid1d((long)ra.NB * ra.Hd * ra.Wd * (ra.C / 4)), 0, ra);
    return 0;
}

// replay the tiled plan for f.NB samples (embedding already evaluated into d_dense); f.x is NCHW, f.out is NCHW
int run_tiled(rdmi_ctx* c, const FwdIn& f, hipStream_t s) {
    const TiledPlan& p = *c->tiled;
    const int HW = c->H * c->W, Cc = c->arch.channels;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, grid1d((long)f.NB * HW * Cc), dim3(RDMI_THREADS), 0, s, f.x, p.xin.get(), f.NB, HW, Cc, f.x_mod);
    TRun R{c, f, s};
    for (const TLaunch& l : p.launches) {
        R.l = &l;
        if (int e = std::visit([&](const auto& r) { return run_launch(R, r); }, l.op)) return e;
        ++R.li;
    }
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, grid1d((long)f.NB * HW * Cc), dim3(RDMI_THREADS), 0, s, (const float*)p.out.get(), f.out, f.NB, HW, Cc, 0);
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace
