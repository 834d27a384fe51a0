// librdmi: host side of the MI355X-native NCSN++ / reflected PC sampler (C ABI in include/rdmi.h).
//
// Structure: rdmi_create() turns the architecture keys into a static LAUNCH PLAN -- a list of fused
// kernels over a liveness-packed NHWC activation workspace -- mirroring the data flow of
// NCSNpp.forward (RD/models/ncsnpp.py:226-354).  Entry points replay the plan on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <climits>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rdmi.h"
#include "attn_kernel.h"
#include "conv_kernel.h"
#include "misc_kernels.h"
#include "unet_kernel.h"
#include "bwd_kernels.h"
#include "opt_kernels.h"
#include "ode_kernels.h"
#include "tiled_kernels.h"

namespace {

thread_local std::string g_err;

int fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

#define HIP_OK(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Owning handles of device memory (and of pinned host memory).  Kernel argument structs keep raw pointers: they are views,
// filled with .get().  Only raw pointers reach hipLaunchKernelGGL.
struct hip_free { void operator()(void* p) const { (void)hipFree(p); } };
struct hip_host_free { void operator()(void* p) const { (void)hipHostFree(p); } };
template <class T> using dev_ptr = std::unique_ptr<T, hip_free>;
template <class T> using pinned_ptr = std::unique_ptr<T, hip_host_free>;

// p = n fresh elements (what p held is released first); used as HIP_OK(hip_alloc(p, n))
template <class T> hipError_t hip_alloc(dev_ptr<T>& p, size_t n) {
    p.reset();
    T* q = nullptr;
    const hipError_t e = hipMalloc((void**)&q, n * sizeof(T));
    if (e == hipSuccess) p.reset(q);
    return e;
}
template <class T> hipError_t hip_alloc(pinned_ptr<T>& p, size_t n) {
    p.reset();
    T* q = nullptr;
    const hipError_t e = hipHostMalloc((void**)&q, n * sizeof(T), 0);
    if (e == hipSuccess) p.reset(q);
    return e;
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int pad16(int a) { return (a + 15) & ~15; }

struct Param {
    std::string name;
    std::vector<int> shape;
    size_t numel = 0;
    const float* ptr = nullptr;
};

struct Tensor {
    std::string name;
    int C = 0, H = 0, W = 0;
    size_t off = 0;           // floats per sample from the workspace base (times max_batch)
    int def = -1, last = -1;  // defining / last-reading op index
    size_t per_sample() const { return (size_t)C * H * W; }
};

// description of one fused conv launch of the layer plan (kept per op: the backward plan is derived from it)
struct ConvSpec {
    std::string name;
    int tA = -1, tB = -1;           // sources (tA == -2: caller's x)
    int CA = 0, CB = 0;
    int Ha = 0, Wa = 0;             // source-A dims
    int Hv = 0, Wv = 0;             // virtual input dims
    std::string gn;                 // GroupNorm param prefix ("" = none)
    std::string conv;               // conv param prefix
    int stride = 1, pad_lo = 1;
    int Ho = 0, Wo = 0, Cout = 0;
    // shortcut
    int tScA = -1, tScB = -1, CscA = 0, CscB = 0, Hsa = 0, Wsa = 0;
    std::string nin;
    int dense_off = -1;
    int tRes = -1;
    float scale = 1.f;
    bool to_output = false;
    bool dropout = false;
};

enum OpKind { OP_CONV, OP_ATTN };

struct Op {
    OpKind kind;
    std::string name;
    ConvArgs conv{};
    AttnArgs attn{};
    int cfg = 0;                 // conv tile configuration
    int out_tensor = -1;
    double flops_per_sample = 0;
    // tensor ids, resolved to pointers once the workspace is allocated
    int tA = -1, tB = -1, tScA = -1, tScB = -1, tRes = -1;
    bool a_is_input = false;     // A source is the caller's x (input_conv)
    bool out_is_output = false;  // writes the caller's out (out_conv)
    bool use_dense = false;      // epilogue adds this block's Dense_0(SiLU(temb)) column slice
    std::vector<int> tab, mapA, mapSc;
    size_t tab_off = 0, mapA_off = 0, mapSc_off = 0;   // into the int arena
    bool has_mapA = false, has_mapSc = false;
    // packed weight locations (floats into the weight arena)
    size_t w_off = 0, wsc_off = 0, w3_off = 0, bqkv_off = 0;
    int p_gamma = -1, p_beta = -1, p_bias = -1, p_bias_sc = -1, p_b3 = -1;   // parameter indices (-1: none), resolved when the plan is built
    ConvSpec spec;               // OP_CONV: what was asked for
    int attn_C = 0, attn_H = 0, attn_W = 0;
    bool dropout = false;        // train mode applies Dropout_0 to this op's activated input (Conv_1 of a resblock)
};

struct ProfEntry { std::string name; double ms = 0; long launches = 0; double flops = 0; };
struct TrainPlan;                        // csrc/train_plan.h
struct TiledPlan;                        // csrc/tiled_plan.h
struct FusedPlan;                        // csrc/fused_plan.h

}  // namespace

struct rdmi_ctx {
    rdmi_arch arch{};
    int max_batch = 0, H = 0, W = 0;
    int temb = 0, dense_total = 0;
    std::vector<Param> params;
    std::map<std::string, int> pindex;
    std::vector<Tensor> tensors;
    std::vector<Op> ops;
    std::vector<PackJob> jobs;          // host copy (src pointers patched from params before upload)
    std::vector<int> job_param;         // param index feeding each job
    std::vector<int> job_param2;        // second source of a job (PackJob::src2), -1: none; filled up to jobs.size() in do_repack
    dev_ptr<PackJob> d_jobs;
    dev_ptr<float> d_w;                 // packed weight arena
    size_t w_floats = 0;
    dev_ptr<int> d_int;                 // tables and pixel maps
    dev_ptr<float> ws;                  // activation workspace
    size_t ws_per_sample = 0;
    // embedding path
    size_t w_t0 = 0, w_t2 = 0, w_dense = 0, b_dense = 0;
    dev_ptr<float> d_h1, d_temb, d_dense;
    // sampler scratch
    dev_ptr<float> d_s2, d_score, d_z, d_norms, d_ts, d_tvec;
    dev_ptr<float> d_tt, d_th1; int tt_cap = 0;                 // sampler: time-path rows of all updates (rdmi_pc_sample)
    dev_ptr<float> d_dense_all; size_t dense_all_cap = 0;      // sampler: Dense_0 outputs of a chunk of updates [U][NBm][dense_total]
    dev_ptr<StepState> d_state;
    bool use_fused = true;               // RDMI_PATH=layers: the layer plan runs although the fused programs exist
    std::unique_ptr<FusedPlan> fused;    // the workgroup-resident programs of a context that does not run the tiled plan (csrc/fused_plan.h)
    std::unique_ptr<TiledPlan> tiled;    // non-null: the context runs the tiled plan (shapes whose samples do not fit one workgroup: csrc/tiled_plan.h)
    bool in_train_forward = false;       // set around run_forward by rdmi_train_forward
    dev_ptr<bf16_t> d_w16;               // bf16 copies of the forward conv weights (training with compute_dtype = bf16)
    float train_drop_p = 0.f; const unsigned long long* train_seed_dev = nullptr;      // set around the training forward's launch
    std::map<std::string, size_t> wmap;  // packed-weight arena offsets by parameter prefix
    bool packed_valid = false;
    bool debug_taps = false;
    bool profiling = false;
    std::vector<ProfEntry> prof;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::vector<int> ev_entry;
    size_t ev_used = 0;
    std::unique_ptr<TrainPlan> train;    // rdmi_enable_training (csrc/train_plan.h)
    ~rdmi_ctx();                         // defined after train_plan.h: TiledPlan, FusedPlan and TrainPlan are complete there
};

namespace {

// ------------------------------------------------------------------------------------------
// parameter list: the reference's state-dict order (RD/models/ncsnpp.py:42-224)
// ------------------------------------------------------------------------------------------
void add_param(rdmi_ctx* c, const std::string& name, std::vector<int> shape) {
    Param p;
    p.name = name;
    p.shape = shape;
    p.numel = 1;
    for (int s : shape) p.numel *= (size_t)s;
    c->pindex[name] = (int)c->params.size();
    c->params.push_back(p);
}
void add_gn(rdmi_ctx* c, const std::string& pre, int ch) { add_param(c, pre + ".weight", {ch}); add_param(c, pre + ".bias", {ch}); }
void add_conv_p(rdmi_ctx* c, const std::string& pre, int cin, int cout) { add_param(c, pre + ".weight", {cout, cin, 3, 3}); add_param(c, pre + ".bias", {cout}); }
void add_nin(rdmi_ctx* c, const std::string& pre, int cin, int cout) { add_param(c, pre + ".W", {cin, cout}); add_param(c, pre + ".b", {cout}); }
void add_resblock_p(rdmi_ctx* c, const std::string& pre, int cin, int cout) {
    add_gn(c, pre + ".GroupNorm_0", cin);
    add_conv_p(c, pre + ".Conv_0", cin, cout);
    add_param(c, pre + ".Dense_0.weight", {cout, c->temb});
    add_param(c, pre + ".Dense_0.bias", {cout});
    add_gn(c, pre + ".GroupNorm_1", cout);
    add_conv_p(c, pre + ".Conv_1", cout, cout);
    if (cin != cout) add_nin(c, pre + ".NIN_0", cin, cout);
}
void add_attn_p(rdmi_ctx* c, const std::string& pre, int ch) {
    add_gn(c, pre + ".GroupNorm_0", ch);
    for (int i = 0; i < 4; ++i) add_nin(c, pre + ".NIN_" + std::to_string(i), ch, ch);
}

struct BlockSpec { std::string name; int cin, cout; bool attn; int level; };

struct Layout {
    std::vector<BlockSpec> down, up;       // in execution order
    std::vector<int> skip_ch;
    int mid_ch = 0;
};

Layout build_layout(rdmi_ctx* c) {
    const rdmi_arch& a = c->arch;
    Layout L;
    int in_ch = a.nf, d = 0;
    for (int i = 0; i < a.n_levels; ++i) {
        const int out_ch = a.nf * a.ch_mult[i];
        for (int j = 0; j < a.num_res_blocks; ++j) {
            L.down.push_back({"down_blocks." + std::to_string(d), in_ch, out_ch, (a.attn_levels >> i & 1) != 0, i});
            in_ch = out_ch;
            L.skip_ch.push_back(in_ch);
            ++d;
        }
        L.skip_ch.push_back(in_ch);
    }
    L.mid_ch = in_ch;
    std::vector<int> sk(L.skip_ch.rbegin(), L.skip_ch.rend());
    int u = 0, k = 0;
    for (int i = a.n_levels - 1; i >= 0; --i) {
        const int out_ch = a.nf * a.ch_mult[i];
        for (int j = 0; j < a.num_res_blocks + 1; ++j) {
            L.up.push_back({"up_blocks." + std::to_string(u), in_ch + sk[k++], out_ch, (a.attn_levels >> i & 1) != 0, i});
            in_ch = out_ch;
            ++u;
        }
    }
    return L;
}

void build_params(rdmi_ctx* c, const Layout& L) {
    const rdmi_arch& a = c->arch;
    add_param(c, "time_embed.W", {a.nf});
    add_param(c, "time_mlp.0.weight", {c->temb, 2 * a.nf});
    add_param(c, "time_mlp.0.bias", {c->temb});
    add_param(c, "time_mlp.2.weight", {c->temb, c->temb});
    add_param(c, "time_mlp.2.bias", {c->temb});
    if (a.conditional) {
        add_param(c, "label_emb.weight", {c->temb, a.num_classes});
        add_param(c, "label_emb.bias", {c->temb});
    }
    add_conv_p(c, "input_conv", a.channels, a.nf);
    for (auto& b : L.down) add_resblock_p(c, b.name, b.cin, b.cout);
    for (size_t i = 0; i < L.down.size(); ++i)
        if (L.down[i].attn) add_attn_p(c, "down_attn." + std::to_string(i), L.down[i].cout);
    {
        int ch = a.nf;
        for (int i = 0; i < a.n_levels; ++i) {
            ch = a.nf * a.ch_mult[i];
            if (i != a.n_levels - 1) add_conv_p(c, "downsample." + std::to_string(i) + ".Conv_0", ch, ch);
        }
    }
    add_resblock_p(c, "mid_block1", L.mid_ch, L.mid_ch);
    add_resblock_p(c, "mid_block2", L.mid_ch, L.mid_ch);
    for (auto& b : L.up) add_resblock_p(c, b.name, b.cin, b.cout);
    for (size_t i = 0; i < L.up.size(); ++i)
        if (L.up[i].attn) add_attn_p(c, "up_attn." + std::to_string(i), L.up[i].cout);
    for (int k = 0, i = a.n_levels - 1; i >= 1; --i, ++k) {
        const int ch = a.nf * a.ch_mult[i];
        add_conv_p(c, "upsample." + std::to_string(k) + ".Conv_0", ch, ch);
    }
    add_gn(c, "out_norm", a.nf * a.ch_mult[0]);
    add_conv_p(c, "out_conv", a.nf * a.ch_mult[0], a.channels);
}

// ------------------------------------------------------------------------------------------
// plan builder
// ------------------------------------------------------------------------------------------
// Shapes for which the 3x3 conv after a nearest-x2 upsample runs folded into four 2x2 phase convs in the inference programs of the
// workgroup-resident kernel (fused_plan.h: FusedBuilder::conv_up4): a 4x4 source (a phase = one 16-row MFMA tile), a square weight, input channels in
// whole groups of 128 (the single-tile tap-major loop with the 8-deep weight ring).  RDMI_NO_UP_FOLD=1 keeps the nine-tap op everywhere.
// Asked by the layer plan (does the folded packing exist?) and by the program builder (does this op fold?): one rule for both.
inline bool up_fold_shape_ok(int Hs, int Ws, int Cin, int Cout) {
    return std::getenv("RDMI_NO_UP_FOLD") == nullptr && Hs * Ws == 16 && Cin == Cout && Cin % 128 == 0;
}

// Attention blocks whose k projection is folded into q in the inference programs (fused_attn): the softmax over keys only sees
// (x M + c) . x^T with M = Wq Wk^T, c = bq Wk^T -- the score terms that depend on the query row alone cancel -- so K is the
// GroupNorm_0 output x itself and the projection op computes q' and the NIN_3-folded v' only.  The fold rides on the NIN_3 fold and on
// the single-pass projection (fconv_qkv: C = 64, at most 96 rows).  RDMI_NO_K_FOLD=1 keeps three projections.
// Asked by the layer plan (does the folded packing exist?) and by the program builder: one rule for both.
inline bool k_fold_shape_ok(int C, int L) {
    return std::getenv("RDMI_NO_K_FOLD") == nullptr && std::getenv("RDMI_NO_ATTN_FOLD") == nullptr && std::getenv("RDMI_NO_QKV1") == nullptr && C == 64 && L <= 96;
}

struct Builder {
    rdmi_ctx* c;
    std::vector<int> ints;       // table / map arena (host)
    size_t wf = 0;               // packed weight floats so far

    int new_tensor(const std::string& name, int C, int H, int W) {
        Tensor t;
        t.name = name; t.C = C; t.H = H; t.W = W;
        t.def = (int)c->ops.size();
        c->tensors.push_back(t);
        return (int)c->tensors.size() - 1;
    }
    void use(int t) { if (t >= 0) c->tensors[t].last = (int)c->ops.size(); }

    size_t alloc_w(size_t n) { size_t o = wf; wf += (n + 63) & ~(size_t)63; return o; }

    void job_pack(const std::string& pname, size_t dst_off, int Cin, int Cout, int Kpad, int Npad, int n_off, int ntap,
                  long s_co, long s_ci, long s_t) {
        PackJob j{};
        j.dst = reinterpret_cast<float*>(dst_off);   // patched to a pointer after the arena exists
        j.Cin = Cin; j.Cout = Cout; j.Kpad = Kpad; j.Npad = Npad; j.n_off = n_off; j.ntap = ntap;
        j.s_co = s_co; j.s_ci = s_ci; j.s_t = s_t; j.kind = 0;
        c->jobs.push_back(j);
        c->job_param.push_back(c->pindex.at(pname));
    }
    void job_copy(const std::string& pname, size_t dst_off, int n, int n_off) {
        PackJob j{};
        j.dst = reinterpret_cast<float*>(dst_off);
        j.Cout = n; j.n_off = n_off; j.kind = 1;
        c->jobs.push_back(j);
        c->job_param.push_back(c->pindex.at(pname));
    }
    // conv weight OIHW -> [9][Kpad/16][Npad][16]
    size_t pack_conv(const std::string& pre, int cin, int cout) {
        const int Kp = pad16(cin), Np = pad16(cout);
        size_t o = alloc_w((size_t)9 * Kp * Np);
        job_pack(pre + ".weight", o, cin, cout, Kp, Np, 0, 9, (long)cin * 9, 9, 1);
        c->wmap[pre] = o;
        return o;
    }
    // NIN W [in][out] -> [Kpad/16][Npad][16]
    size_t pack_nin(const std::string& pre, int cin, int cout) {
        const int Kp = pad16(cin), Np = pad16(cout);
        size_t o = alloc_w((size_t)Kp * Np);
        job_pack(pre + ".W", o, cin, cout, Kp, Np, 0, 1, 1, cout, 0);
        c->wmap[pre] = o;
        return o;
    }

    static std::vector<int> nearest_map(int Hs, int Ws, int Hd, int Wd) {
        // F.interpolate(mode='nearest'): src = floor(dst * in / out)   (RD/models/ncsnpp.py:320, layerspp.py:122)
        std::vector<int> m((size_t)Hd * Wd);
        for (int y = 0; y < Hd; ++y)
            for (int x = 0; x < Wd; ++x) {
                int sy = std::min((int)std::floor(y * ((float)Hs / Hd)), Hs - 1);
                int sx = std::min((int)std::floor(x * ((float)Ws / Wd)), Ws - 1);
                m[(size_t)y * Wd + x] = sy * Ws + sx;
            }
        return m;
    }

    int add_conv(const ConvSpec& s, int* err) {
        Op op;
        op.kind = OP_CONV;
        op.name = s.name;
        ConvArgs& a = op.conv;
        const int Cin = s.CA + s.CB;
        a.CA = s.CA; a.CB = s.CB; a.Cv = pad16(Cin);
        a.HWa = s.Ha * s.Wa; a.HWv = s.Hv * s.Wv; a.HWo = s.Ho * s.Wo;
        a.ntap = 9;
        a.G = s.gn.empty() ? 0 : std::min(Cin / 4, 32);
        a.Cout = s.Cout; a.Cout_pad = pad16(s.Cout);
        a.out_scale = s.scale; a.eps = 1e-6f;
        a.dense_stride = c->dense_total; a.dense_off = s.dense_off < 0 ? 0 : s.dense_off;
        a.CscA = s.CscA; a.CscB = s.CscB; a.Csc = pad16(s.CscA + s.CscB) * ((s.CscA + s.CscB) > 0);
        a.HWsa = s.Hsa * s.Wsa;
        op.tA = s.tA; op.tB = s.tB; op.tScA = s.tScA; op.tScB = s.tScB; op.tRes = s.tRes;
        op.a_is_input = (s.tA == -2);
        op.out_is_output = s.to_output;
        op.use_dense = s.dense_off >= 0;
        op.spec = s;
        op.dropout = s.dropout;
        // tile configuration
        if (a.Cout_pad < 32) { op.cfg = 3; a.S = 1; a.BN = 16; }                   // <4,1,1,2,1>
        else if (a.HWo >= 40) { op.cfg = 0; a.S = 1; a.BN = 64; }                  // <1,4,1,6,1>
        else if (a.HWo >= 9) { op.cfg = 1; a.S = std::max(1, 64 / a.HWo); a.BN = 32; }   // <2,2,1,3,1>
        else { op.cfg = 2; a.S = std::max(1, 16 / a.HWo); a.BN = 32; }             // <1,2,2,1,1>
        a.Mpad = pad16(a.S * a.HWo);
        const int cap[4] = {96, 96, 16, 128};
        if (a.Mpad > cap[op.cfg] || a.Cout_pad % a.BN != 0 || (op.cfg == 2 && (a.Cv >> 4) < 2)) { *err = fail("conv %s: unsupported tile (HWo=%d Cout=%d)", s.name.c_str(), a.HWo, a.Cout); return -1; }
        if (a.G > 0) {
            const int pairs = a.S * a.G;
            if (a.Cv != Cin || Cin % a.G != 0 || pairs > 256 || (pairs & (pairs - 1)) != 0) { *err = fail("conv %s: unsupported GroupNorm shape C=%d", s.name.c_str(), Cin); return -1; }
        }
        if (s.CA % 4 != 0 && s.CB != 0) { *err = fail("conv %s: unaligned concat", s.name.c_str()); return -1; }
        if (conv_lds_bytes(a) > 160 * 1024) { *err = fail("conv %s: LDS tile %zu B too large", s.name.c_str(), conv_lds_bytes(a)); return -1; }
        // tap table: row m = s*HWo + (oy*Wo + ox) -> LDS row s*HWv + iy*Wv + ix, or the zero row
        const int zrow = a.S * a.HWv, zrow_sc = a.S * a.HWo;
        op.tab.assign((size_t)a.Mpad * 10, zrow);
        for (int m = 0; m < a.Mpad; ++m) {
            const int sidx = m / a.HWo, p = m % a.HWo;
            const bool real = m < a.S * a.HWo;
            const int oy = p / s.Wo, ox = p % s.Wo;
            for (int t = 0; t < 9; ++t) {
                const int iy = oy * s.stride + t / 3 - s.pad_lo, ix = ox * s.stride + t % 3 - s.pad_lo;
                if (real && iy >= 0 && iy < s.Hv && ix >= 0 && ix < s.Wv) op.tab[(size_t)m * 10 + t] = sidx * a.HWv + iy * s.Wv + ix;
            }
            op.tab[(size_t)m * 10 + 9] = real ? m : zrow_sc;
        }
        if (s.Ha != s.Hv || s.Wa != s.Wv) { op.mapA = nearest_map(s.Ha, s.Wa, s.Hv, s.Wv); op.has_mapA = true; }
        if (a.Csc && (s.Hsa != s.Ho || s.Wsa != s.Wo)) { op.mapSc = nearest_map(s.Hsa, s.Wsa, s.Ho, s.Wo); op.has_mapSc = true; }
        op.tab_off = ints.size(); ints.insert(ints.end(), op.tab.begin(), op.tab.end());
        if (op.has_mapA) { op.mapA_off = ints.size(); ints.insert(ints.end(), op.mapA.begin(), op.mapA.end()); }
        if (op.has_mapSc) { op.mapSc_off = ints.size(); ints.insert(ints.end(), op.mapSc.begin(), op.mapSc.end()); }
        // weights
        op.w_off = pack_conv(s.conv, Cin, s.Cout);
        op.p_bias = c->pindex.at(s.conv + ".bias");
        if (!s.gn.empty()) { op.p_gamma = c->pindex.at(s.gn + ".weight"); op.p_beta = c->pindex.at(s.gn + ".bias"); }
        if (a.Csc) { op.wsc_off = pack_nin(s.nin, s.CscA + s.CscB, s.Cout); op.p_bias_sc = c->pindex.at(s.nin + ".b"); }
        op.flops_per_sample = 2.0 * a.HWo * s.Cout * (9.0 * Cin + (s.CscA + s.CscB));
        use(s.tA); use(s.tB); use(s.tScA); use(s.tScB); use(s.tRes);
        int out = -1;
        if (!s.to_output) { out = new_tensor(s.name, s.Cout, s.Ho, s.Wo); }
        op.out_tensor = out;
        c->ops.push_back(op);
        return out;
    }

    int add_attn(const std::string& name, int tin, int C, int H, int W, int* err) {
        Op op;
        op.kind = OP_ATTN;
        op.name = name;
        if (C != 64 || H * W > 96) { *err = fail("attention %s: only C=64, H*W<=96 is built (got C=%d, L=%d)", name.c_str(), C, H * W); return -1; }
        AttnArgs& a = op.attn;
        a.L = H * W; a.Lpad = pad16(a.L); a.G = std::min(C / 4, 32);
        a.eps = 1e-6f; a.scale = 1.0f / std::sqrt((float)C); a.out_scale = (float)(1.0 / std::sqrt(2.0));
        op.tA = tin;
        op.w_off = alloc_w((size_t)3 * C * C);
        for (int i = 0; i < 3; ++i) {
            PackJob j{};
            j.dst = reinterpret_cast<float*>(op.w_off + (size_t)i * C * C);
            j.Cin = C; j.Cout = C; j.Kpad = C; j.Npad = C; j.n_off = 0; j.ntap = 1; j.s_co = 1; j.s_ci = C; j.s_t = 0; j.kind = 0;
            c->jobs.push_back(j);
            c->job_param.push_back(c->pindex.at(name + ".NIN_" + std::to_string(i) + ".W"));
        }
        c->wmap[name + ".qkv"] = op.w_off;
        {   // fused-plan packing: q|k|v side by side as one [C/16][3C][16] matrix
            const size_t o3 = alloc_w((size_t)3 * C * C);
            for (int i = 0; i < 3; ++i) {
                PackJob j{};
                j.dst = reinterpret_cast<float*>(o3);
                j.Cin = C; j.Cout = C; j.Kpad = C; j.Npad = 3 * C; j.n_off = i * C; j.ntap = 1; j.s_co = 1; j.s_ci = C; j.s_t = 0; j.kind = 0;
                c->jobs.push_back(j);
                c->job_param.push_back(c->pindex.at(name + ".NIN_" + std::to_string(i) + ".W"));
            }
            c->wmap[name + ".qkv3"] = o3;
        }
        {   // the same block with NIN_3 folded into the value projection: softmax(QK^T) (V W3) == (softmax(QK^T) V) W3, so the inference
            // programs of the workgroup-resident kernel run no NIN_3 op at all (fused_attn); v-columns = NIN_2.W x NIN_3.W, v-bias = NIN_2.b x NIN_3.W
            const size_t o3 = alloc_w((size_t)3 * C * C);
            for (int i = 0; i < 3; ++i) {
                PackJob j{};
                j.dst = reinterpret_cast<float*>(o3);
                j.Cin = C; j.Cout = C; j.Kpad = C; j.Npad = 3 * C; j.n_off = i * C; j.ntap = 1; j.s_co = 1; j.s_ci = C; j.s_t = 0; j.kind = i == 2 ? 3 : 0;
                c->jobs.push_back(j);
                c->job_param.push_back(c->pindex.at(name + ".NIN_" + std::to_string(i) + ".W"));
                c->job_param2.resize(c->jobs.size(), -1);
                if (i == 2) c->job_param2.back() = c->pindex.at(name + ".NIN_3.W");
            }
            c->wmap[name + ".qkv3f"] = o3;
            const size_t ob = alloc_w((size_t)3 * C);
            c->wmap[name + ".bqkvf"] = ob;
            for (int i = 0; i < 2; ++i) job_copy(name + ".NIN_" + std::to_string(i) + ".b", ob, C, i * C);
            PackJob j{};
            j.dst = reinterpret_cast<float*>(ob);
            j.Cin = C; j.Cout = C; j.n_off = 2 * C; j.kind = 4;
            c->jobs.push_back(j);
            c->job_param.push_back(c->pindex.at(name + ".NIN_2.b"));
            c->job_param2.resize(c->jobs.size(), -1);
            c->job_param2.back() = c->pindex.at(name + ".NIN_3.W");
        }
        if (k_fold_shape_ok(C, a.L)) {   // q' | v' side by side as [C/16][2C][16]: q' = NIN_0.W x NIN_1.W^T with bias NIN_0.b x NIN_1.W^T (the k projection folded
            // into q, see k_fold_shape_ok), v' as in ".qkv3f".  Products formed on the device at every repack, k ascending.
            const size_t o2 = alloc_w((size_t)2 * C * C), ob = alloc_w((size_t)2 * C);
            c->wmap[name + ".qv2f"] = o2;
            c->wmap[name + ".bqvf"] = ob;
            for (int i = 0; i < 2; ++i) {
                PackJob j{};
                j.dst = reinterpret_cast<float*>(o2);
                j.Cin = C; j.Cout = C; j.Kpad = C; j.Npad = 2 * C; j.n_off = i * C; j.ntap = 1; j.s_co = 1; j.s_ci = C; j.s_t = 0; j.kind = i == 0 ? 6 : 3;
                c->jobs.push_back(j);
                c->job_param.push_back(c->pindex.at(name + (i == 0 ? ".NIN_0.W" : ".NIN_2.W")));
                c->job_param2.resize(c->jobs.size(), -1);
                c->job_param2.back() = c->pindex.at(name + (i == 0 ? ".NIN_1.W" : ".NIN_3.W"));
                PackJob v{};
                v.dst = reinterpret_cast<float*>(ob);
                v.Cin = C; v.Cout = C; v.n_off = i * C; v.kind = i == 0 ? 7 : 4;
                c->jobs.push_back(v);
                c->job_param.push_back(c->pindex.at(name + (i == 0 ? ".NIN_0.b" : ".NIN_2.b")));
                c->job_param2.resize(c->jobs.size(), -1);
                c->job_param2.back() = c->pindex.at(name + (i == 0 ? ".NIN_1.W" : ".NIN_3.W"));
            }
        }
        op.bqkv_off = alloc_w((size_t)3 * C);
        c->wmap[name + ".bqkv"] = op.bqkv_off;
        for (int i = 0; i < 3; ++i) job_copy(name + ".NIN_" + std::to_string(i) + ".b", op.bqkv_off, C, i * C);
        op.w3_off = pack_nin(name + ".NIN_3", C, C);
        op.p_b3 = c->pindex.at(name + ".NIN_3.b");
        op.p_gamma = c->pindex.at(name + ".GroupNorm_0.weight"); op.p_beta = c->pindex.at(name + ".GroupNorm_0.bias");
        op.flops_per_sample = 2.0 * (4.0 * a.L * C * C + 2.0 * a.L * a.L * C);
        op.attn_C = C; op.attn_H = H; op.attn_W = W;
        use(tin);
        const int out = new_tensor(name, C, H, W);
        op.out_tensor = out;
        c->ops.push_back(op);
        return out;
    }
};

// one ResnetBlockDDPMpp = two fused conv launches
int add_resblock(Builder& b, const std::string& name, int tA, int tB, int CA, int CB, int Ha, int Wa, int H, int W,
                 int cout, int dense_off, int* err) {
    ConvSpec s0;
    s0.name = name + ".Conv_0";
    s0.tA = tA; s0.tB = tB; s0.CA = CA; s0.CB = CB; s0.Ha = Ha; s0.Wa = Wa; s0.Hv = H; s0.Wv = W;
    s0.gn = name + ".GroupNorm_0"; s0.conv = name + ".Conv_0";
    s0.Ho = H; s0.Wo = W; s0.Cout = cout; s0.dense_off = dense_off;
    const int h1 = b.add_conv(s0, err);
    if (*err) return -1;
    ConvSpec s1;
    s1.name = name;
    s1.tA = h1; s1.CA = cout; s1.Ha = H; s1.Wa = W; s1.Hv = H; s1.Wv = W;
    s1.gn = name + ".GroupNorm_1"; s1.conv = name + ".Conv_1";
    s1.Ho = H; s1.Wo = W; s1.Cout = cout;
    s1.scale = (float)(1.0 / std::sqrt(2.0));
    s1.dropout = true;
    if (CA + CB != cout) {
        s1.tScA = tA; s1.tScB = tB; s1.CscA = CA; s1.CscB = CB; s1.Hsa = Ha; s1.Wsa = Wa; s1.nin = name + ".NIN_0";
    } else {
        if (tB >= 0 || Ha != H || Wa != W) { *err = fail("%s: identity shortcut over a gathered input is not built", name.c_str()); return -1; }
        s1.tRes = tA;
    }
    return b.add_conv(s1, err);
}


// the tiled plan (csrc/tiled_plan.h, included ahead of run_forward): shapes beyond one workgroup per sample
int build_tiled_plan(rdmi_ctx* c, Builder& b, const Layout& L, std::map<std::string, int>& dense_off);
int finish_tiled_plan(rdmi_ctx* c);
void tiled_bind_params(rdmi_ctx* c);
int build_fused_program(rdmi_ctx* c, const std::map<std::string, int>& dense_off);   // csrc/fused_plan.h

// the device buffers both plans share: weight arena (wf floats, zeroed), pack-job table, embedding rows, sampler scratch
int alloc_arenas(rdmi_ctx* c, size_t wf) {
    const size_t NBm = (size_t)c->max_batch, Mp = (size_t)pad16(c->max_batch), T = (size_t)c->temb;
    const size_t E = (size_t)c->H * c->W * c->arch.channels;
    c->w_floats = wf;
    HIP_OK(hip_alloc(c->d_w, wf));
    HIP_OK(hipMemset(c->d_w.get(), 0, wf * sizeof(float)));
    HIP_OK(hip_alloc(c->d_jobs, c->jobs.size()));
    HIP_OK(hip_alloc(c->d_h1, Mp * T));
    HIP_OK(hip_alloc(c->d_temb, Mp * T));
    HIP_OK(hip_alloc(c->d_dense, Mp * c->dense_total));
    HIP_OK(hip_alloc(c->d_s2, NBm * E));
    HIP_OK(hip_alloc(c->d_score, NBm * E));
    HIP_OK(hip_alloc(c->d_z, NBm * E));
    HIP_OK(hip_alloc(c->d_norms, 2 * NBm + 2));
    HIP_OK(hip_alloc(c->d_tvec, NBm));
    HIP_OK(hip_alloc(c->d_state, 1));
    HIP_OK(hipMemset(c->d_state.get(), 0, sizeof(StepState)));
    for (auto& j : c->jobs) j.dst = c->d_w.get() + reinterpret_cast<size_t>(j.dst);
    return 0;
}

int build_plan(rdmi_ctx* c) {
    const rdmi_arch& a = c->arch;
    Layout L = build_layout(c);
    build_params(c, L);
    // every GroupNorm has G = min(C / 4, 32) groups (RD/models/layerspp.py) and every plan computes Cg = C / G: a C that G does not divide
    // (nf 48 with ch_mult [1, 2, 2]: the 144-channel concat, G = 32) is refused by torch.nn.GroupNorm and would silently drop channels here
    for (const Param& p : c->params) {
        const bool gn_w = p.name == "out_norm.weight" || (p.name.find(".GroupNorm_") != std::string::npos && p.name.size() > 7 &&
                                                          p.name.compare(p.name.size() - 7, 7, ".weight") == 0);
        if (!gn_w) continue;
        const int C = (int)p.numel, G = std::min(C / 4, 32);
        if (G < 1 || C % G != 0)
            return fail("%s: GroupNorm over %d channels in min(C / 4, 32) = %d groups: num_channels must be divisible by num_groups",
                        p.name.substr(0, p.name.size() - 7).c_str(), C, G);
    }
    Builder b{c};
    int err = 0;
    // Dense_0 offsets in block order (down, mid1, mid2, up)
    std::vector<std::pair<std::string, int>> dense_blocks;
    for (auto& d : L.down) dense_blocks.push_back({d.name, d.cout});
    dense_blocks.push_back({"mid_block1", L.mid_ch});
    dense_blocks.push_back({"mid_block2", L.mid_ch});
    for (auto& u : L.up) dense_blocks.push_back({u.name, u.cout});
    std::map<std::string, int> dense_off;
    int dt = 0;
    for (auto& d : dense_blocks) { dense_off[d.first] = dt; dt += d.second; }
    c->dense_total = dt;

    // embedding weights: time_mlp.0 [temb][2nf], time_mlp.2 [temb][temb], all Dense_0 side by side
    const int T = c->temb, Np_d = (dt + 63) & ~63, Np_t = (T + 63) & ~63;
    c->w_t0 = b.alloc_w((size_t)pad16(2 * a.nf) * Np_t);
    b.job_pack("time_mlp.0.weight", c->w_t0, 2 * a.nf, T, pad16(2 * a.nf), Np_t, 0, 1, 2 * a.nf, 1, 0);
    c->w_t2 = b.alloc_w((size_t)T * Np_t);
    b.job_pack("time_mlp.2.weight", c->w_t2, T, T, T, Np_t, 0, 1, T, 1, 0);
    c->w_dense = b.alloc_w((size_t)T * Np_d);
    c->b_dense = b.alloc_w((size_t)Np_d);
    for (auto& d : dense_blocks) {
        b.job_pack(d.first + ".Dense_0.weight", c->w_dense, T, d.second, T, Np_d, dense_off[d.first], 1, T, 1, 0);
        b.job_copy(d.first + ".Dense_0.bias", c->b_dense, d.second, dense_off[d.first]);
    }

    // Shapes beyond one workgroup per sample (more than 96 pixels, or more than one image channel: the CIFAR-shape model of
    // BASELINE config #5) run the spatially tiled plan; the GTO-Halo shapes keep the workgroup-resident / layer plans below.
    if (a.compute_dtype != 0 && a.compute_dtype != 1) return fail("compute_dtype=%d (0: fp32, 1: bf16)", a.compute_dtype);
    if (c->H * c->W > 96 || a.channels != 1) {
        try { if (int e = build_tiled_plan(c, b, L, dense_off)) return e; }
        catch (const std::exception& ex) { return fail("tiled plan: %s", ex.what()); }
        if (int e = alloc_arenas(c, b.wf)) return e;
        return finish_tiled_plan(c);
    }
    // ---- NCSNpp.forward data flow
    int H = c->H, W = c->W;
    ConvSpec in;
    in.name = "input_conv"; in.tA = -2; in.CA = a.channels; in.Ha = H; in.Wa = W; in.Hv = H; in.Wv = W;
    in.conv = "input_conv"; in.Ho = H; in.Wo = W; in.Cout = a.nf;
    int h = b.add_conv(in, &err);
    if (err) return err;
    struct HS { int t, C, H, W; };
    std::vector<HS> hs{{h, a.nf, H, W}};
    int ch = a.nf, d = 0;
    for (int i = 0; i < a.n_levels; ++i) {
        for (int j = 0; j < a.num_res_blocks; ++j, ++d) {
            const BlockSpec& bs = L.down[d];
            h = add_resblock(b, bs.name, h, -1, bs.cin, 0, H, W, H, W, bs.cout, dense_off[bs.name], &err);
            if (err) return err;
            ch = bs.cout;
            if (bs.attn) { h = b.add_attn("down_attn." + std::to_string(d), h, ch, H, W, &err); if (err) return err; }
            hs.push_back({h, ch, H, W});
        }
        hs.push_back({h, ch, H, W});
        if (i != a.n_levels - 1) {
            ConvSpec s;
            s.name = "downsample." + std::to_string(i);
            s.tA = h; s.CA = ch; s.Ha = H; s.Wa = W; s.Hv = H; s.Wv = W;
            s.conv = s.name + ".Conv_0"; s.stride = 2; s.pad_lo = 0;
            s.Ho = (H + 1 - 3) / 2 + 1; s.Wo = (W + 1 - 3) / 2 + 1; s.Cout = ch;
            h = b.add_conv(s, &err);
            if (err) return err;
            H = s.Ho; W = s.Wo;
        }
    }
    h = add_resblock(b, "mid_block1", h, -1, ch, 0, H, W, H, W, ch, dense_off["mid_block1"], &err);
    if (err) return err;
    h = add_resblock(b, "mid_block2", h, -1, ch, 0, H, W, H, W, ch, dense_off["mid_block2"], &err);
    if (err) return err;
    int u = 0;
    for (int k = 0; k < a.n_levels; ++k) {
        for (int j = 0; j < a.num_res_blocks + 1; ++j, ++u) {
            const BlockSpec& bs = L.up[u];
            HS sk = hs.back();
            hs.pop_back();
            // h is gathered (nearest) onto the skip's grid when the shapes differ (RD/models/ncsnpp.py:319-320)
            const int Hs = H, Ws = W;
            H = sk.H; W = sk.W;
            h = add_resblock(b, bs.name, h, sk.t, ch, sk.C, Hs, Ws, H, W, bs.cout, dense_off[bs.name], &err);
            if (err) return err;
            ch = bs.cout;
            if (bs.attn) { h = b.add_attn("up_attn." + std::to_string(u), h, ch, H, W, &err); if (err) return err; }
        }
        if (k != a.n_levels - 1) {
            ConvSpec s;
            s.name = "upsample." + std::to_string(k);
            s.tA = h; s.CA = ch; s.Ha = H; s.Wa = W; s.Hv = 2 * H; s.Wv = 2 * W;
            s.conv = s.name + ".Conv_0"; s.Ho = 2 * H; s.Wo = 2 * W; s.Cout = ch;
            h = b.add_conv(s, &err);
            if (err) return err;
            if (k == a.n_levels - 2 && up_fold_shape_ok(H, W, ch, ch)) {      // the upsample onto level 0, folded: 4 phases x 4 pre-summed taps (inference programs of the workgroup-resident kernel)
                const int Kp = pad16(ch), Np = pad16(ch);
                const size_t o = b.alloc_w((size_t)16 * Kp * Np);
                b.job_pack(s.conv + ".weight", o, ch, ch, Kp, Np, 0, 16, (long)ch * 9, 9, 1);
                c->jobs.back().kind = 5;
                c->wmap[s.conv + ".up4"] = o;
            }
            H *= 2; W *= 2;
        }
    }
    if (H != c->H || W != c->W) return fail("network output grid %dx%d != input %dx%d", H, W, c->H, c->W);
    ConvSpec out;
    out.name = "out_conv"; out.tA = h; out.CA = ch; out.Ha = H; out.Wa = W; out.Hv = H; out.Wv = W;
    out.gn = "out_norm"; out.conv = "out_conv"; out.Ho = H; out.Wo = W; out.Cout = a.channels; out.to_output = true;
    b.add_conv(out, &err);
    if (err) return err;

    // ---- liveness-packed workspace offsets
    {
        struct Blk { size_t off, size; };
        std::vector<Blk> freel;
        std::vector<std::vector<int>> dies((size_t)c->ops.size() + 1);
        for (size_t t = 0; t < c->tensors.size(); ++t) {
            Tensor& tt = c->tensors[t];
            if (tt.last < tt.def) tt.last = tt.def;
            dies[(size_t)tt.last].push_back((int)t);
        }
        size_t top = 0;
        size_t ti = 0;
        for (size_t o = 0; o < c->ops.size(); ++o) {
            // tensors defined by op o are allocated before tensors dying at o are released (an op never aliases in/out)
            for (; ti < c->tensors.size() && c->tensors[ti].def == (int)o; ++ti) {
                Tensor& tt = c->tensors[ti];
                const size_t need = (tt.per_sample() + 63) & ~(size_t)63;
                int best = -1;
                if (!c->debug_taps)
                    for (size_t f = 0; f < freel.size(); ++f)
                        if (freel[f].size >= need && (best < 0 || freel[f].size < freel[(size_t)best].size)) best = (int)f;
                if (best >= 0) {
                    tt.off = freel[(size_t)best].off;
                    if (freel[(size_t)best].size > need) { freel[(size_t)best].off += need; freel[(size_t)best].size -= need; }
                    else freel.erase(freel.begin() + best);
                } else { tt.off = top; top += need; }
            }
            for (int t : dies[o]) {
                const Tensor& tt = c->tensors[(size_t)t];
                freel.push_back({tt.off, (tt.per_sample() + 63) & ~(size_t)63});
            }
        }
        c->ws_per_sample = top;
    }

    // ---- device allocations
    if (int e = alloc_arenas(c, b.wf)) return e;
    HIP_OK(hip_alloc(c->d_int, std::max<size_t>(b.ints.size(), 1)));
    HIP_OK(hipMemcpy(c->d_int.get(), b.ints.data(), b.ints.size() * sizeof(int), hipMemcpyHostToDevice));
    const size_t NBmax = (size_t)c->max_batch;
    HIP_OK(hip_alloc(c->ws, c->ws_per_sample * NBmax));

    // ---- resolve pointers that do not depend on parameters
    float* const w = c->d_w.get();
    int* const ints = c->d_int.get();
    for (auto& op : c->ops) {
        auto tptr = [&](int t) -> float* { return t >= 0 ? c->ws.get() + c->tensors[(size_t)t].off * NBmax : nullptr; };
        if (op.kind == OP_CONV) {
            ConvArgs& ca = op.conv;
            ca.srcA = tptr(op.tA); ca.srcB = tptr(op.tB); ca.scA = tptr(op.tScA); ca.scB = tptr(op.tScB);
            ca.resid = tptr(op.tRes);
            ca.out = tptr(op.out_tensor);
            ca.tab = ints + op.tab_off;
            ca.mapA = op.has_mapA ? ints + op.mapA_off : nullptr;
            ca.mapSc = op.has_mapSc ? ints + op.mapSc_off : nullptr;
            ca.wpk = w + op.w_off;
            ca.wsc = ca.Csc ? w + op.wsc_off : nullptr;
            ca.dense = op.use_dense ? c->d_dense.get() : nullptr;
        } else {
            AttnArgs& aa = op.attn;
            aa.x = tptr(op.tA); aa.out = tptr(op.out_tensor);
            aa.wqkv = w + op.w_off; aa.bqkv = w + op.bqkv_off; aa.w3 = w + op.w3_off;
        }
    }
    return build_fused_program(c, dense_off);
}

// ------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------
struct ProfScope {
    rdmi_ctx* c; hipStream_t s; int entry = -1; size_t slot = 0;
    ProfScope(rdmi_ctx* c_, hipStream_t s_, const std::string& name, double flops) : c(c_), s(s_) {
        if (!c->profiling) return;
        for (size_t i = 0; i < c->prof.size(); ++i) if (c->prof[i].name == name) entry = (int)i;
        if (entry < 0) { c->prof.push_back({name, 0, 0, 0}); entry = (int)c->prof.size() - 1; }
        c->prof[(size_t)entry].flops += flops;
        if (c->ev_used == c->ev_pool.size()) {
            hipEvent_t a, b;
            hipEventCreate(&a); hipEventCreate(&b);
            c->ev_pool.push_back({a, b});
            c->ev_entry.push_back(0);
        }
        slot = c->ev_used++;
        c->ev_entry[slot] = entry;
        hipEventRecord(c->ev_pool[slot].first, s);
    }
    ~ProfScope() { if (entry >= 0) hipEventRecord(c->ev_pool[slot].second, s); }
};

void prof_collect(rdmi_ctx* c) {
    for (size_t i = 0; i < c->ev_used; ++i) {
        hipEventSynchronize(c->ev_pool[i].second);
        float ms = 0;
        hipEventElapsedTime(&ms, c->ev_pool[i].first, c->ev_pool[i].second);
        ProfEntry& e = c->prof[(size_t)c->ev_entry[i]];
        e.ms += ms; e.launches += 1;
    }
    c->ev_used = 0;
}

template <int WM, int WN, int WK, int MT, int NT, int PF, bool BF16>
int launch_conv_t(const ConvArgs& a, hipStream_t s) {
    static bool attr_set = false;
    auto k = conv_mfma_kernel<WM, WN, WK, MT, NT, PF, BF16>;
    if (!attr_set) { HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); attr_set = true; }
    dim3 grid((unsigned)ceil_div(a.NB, a.S), (unsigned)(a.Cout_pad / a.BN));
    hipLaunchKernelGGL(k, grid, dim3(RDMI_THREADS), conv_lds_bytes(a), s, a);
    HIP_OK(hipGetLastError());
    return 0;
}

int launch_conv(int cfg, const ConvArgs& a_in, hipStream_t s) {
    ConvArgs a = a_in;
    // Small batches: a launch of one 64-column tile per sample leaves CUs idle (B = 128 at 9x9: 128 workgroups on 256 CUs).  The
    // <2,2,1,3,1> configuration computes the same rows with 32-column tiles -- twice the workgroups, same tables (S = 1, Mpad <= 96).
    static const int split_below = [] { const char* e = std::getenv("RDMI_CONV_SPLIT_BELOW"); return e ? atoi(e) : 200; }();
    if (cfg == 0 && a.S == 1 && a.Mpad <= 96 && (a.Cout_pad % 32) == 0 && ceil_div(a.NB, a.S) * (a.Cout_pad / a.BN) < split_below) { cfg = 1; a.BN = 32; }
    if (a.bf16) {
        if ((a.Cv & 31) || (a.Csc & 31)) return fail("bf16 conv launch with %d / %d input channels (multiples of 32 needed)", a.Cv, a.Csc);
        switch (cfg) {
            case 0: return launch_conv_t<1, 4, 1, 6, 1, 2, true>(a, s);
            case 1: return launch_conv_t<2, 2, 1, 3, 1, 3, true>(a, s);
            case 2: return launch_conv_t<1, 2, 2, 1, 1, 6, true>(a, s);
            case 3: return launch_conv_t<4, 1, 1, 2, 1, 4, true>(a, s);
        }
        return fail("bad conv cfg %d", cfg);
    }
    switch (cfg) {
        case 0: return launch_conv_t<1, 4, 1, 6, 1, 2, false>(a, s);
        case 1: return launch_conv_t<2, 2, 1, 3, 1, 3, false>(a, s);
        case 2: return launch_conv_t<1, 2, 2, 1, 1, 6, false>(a, s);
        case 3: return launch_conv_t<4, 1, 1, 2, 1, 4, false>(a, s);
    }
    return fail("bad conv cfg %d", cfg);
}

const char* cfg_name(int cfg) {
    static const char* n[] = {"conv_mfma<1,4,1,6,1>", "conv_mfma<2,2,1,3,1>", "conv_mfma<1,2,2,1,1>", "conv_mfma<4,1,1,2,1>"};
    return n[cfg];
}

int launch_attn(const AttnArgs& a, hipStream_t s) {
    static bool attr_set = false;
    auto k = attn_mfma_kernel<64>;
    if (!attr_set) { HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); attr_set = true; }
    hipLaunchKernelGGL(k, dim3((unsigned)a.NB), dim3(RDMI_THREADS), attn_lds_bytes<64>(a.Lpad, a.G), s, a);
    HIP_OK(hipGetLastError());
    return 0;
}

const float* P(rdmi_ctx* c, const std::string& name) { return c->params[(size_t)c->pindex.at(name)].ptr; }

struct FwdIn {
    const float* x; int x_mod;            // x holds x_mod samples; sample n reads x[n % x_mod] (0: n)
    const float* sig; int sig_mod;        // sigma or t per sample (n % sig_mod); null: every sample uses t_scalar
    float t_scalar;
    int t_is_time; float smin, ratio;
    const float* labels; int label_rows;
    float* out; int NB;
    const float* tt_row = nullptr;        // sampler: precomputed time_mlp.2 output row (+ both biases) of this evaluation's t
    const float* dense_rows = nullptr;    // sampler: precomputed Dense_0 outputs [NB][dense_total] of this evaluation (skips the whole embedding)
    float drop_p = 0.f; const unsigned long long* seed_dev = nullptr;   // tiled training forward: Dropout_0 probability and the step's seed word (null: no dropout)
};

}  // namespace
#include "tiled_plan.h"
#include "fused_plan.h"
namespace {

// parameter-dependent pointers of the layer plan (every repack, every training step whose parameter storage moved)
void bind_layer_params(rdmi_ctx* c) {
    auto at = [&](int i) -> const float* { return i >= 0 ? c->params[(size_t)i].ptr : nullptr; };
    for (auto& op : c->ops) {
        if (op.kind == OP_CONV) { ConvArgs& a = op.conv; a.bias = at(op.p_bias); a.bias_sc = at(op.p_bias_sc); a.gamma = at(op.p_gamma); a.beta = at(op.p_beta); }
        else { op.attn.gamma = at(op.p_gamma); op.attn.beta = at(op.p_beta); op.attn.b3 = at(op.p_b3); }
    }
}

int do_repack(rdmi_ctx* c, hipStream_t s) {
    for (size_t i = 0; i < c->jobs.size(); ++i) {
        const Param& p = c->params[(size_t)c->job_param[i]];
        if (!p.ptr) return fail("parameter '%s' was never bound (rdmi_set_param)", p.name.c_str());
        c->jobs[i].src = p.ptr;
        const int p2 = i < c->job_param2.size() ? c->job_param2[i] : -1;
        c->jobs[i].src2 = p2 >= 0 ? c->params[(size_t)p2].ptr : nullptr;
        if (p2 >= 0 && !c->jobs[i].src2) return fail("parameter '%s' was never bound (rdmi_set_param)", c->params[(size_t)p2].name.c_str());
    }
    for (auto& p : c->params)
        if (!p.ptr) return fail("parameter '%s' was never bound (rdmi_set_param)", p.name.c_str());
    HIP_OK(hipMemcpyAsync(c->d_jobs.get(), c->jobs.data(), c->jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice, s));
    {
        ProfScope ps(c, s, "pack_kernel", 0);
        hipLaunchKernelGGL(pack_kernel, dim3(32, (unsigned)c->jobs.size()), dim3(RDMI_THREADS), 0, s, (const PackJob*)c->d_jobs.get());
    }
    HIP_OK(hipGetLastError());
    bind_layer_params(c);
    if (c->tiled) tiled_bind_params(c);
    if (c->fused) for (auto& q : c->fused->progs) if (q.ok) if (int e = bind_fused_params(c, q, s)) return e;
    if (fused_ready(c)) HIP_OK(hipStreamSynchronize(s));
    c->packed_valid = true;
    return 0;
}

int run_forward(rdmi_ctx* c, const FwdIn& f, hipStream_t s) {
    const rdmi_arch& a = c->arch;
    if (f.NB < 1 || f.NB > c->max_batch) return fail("batch %d outside [1, %d] (rdmi_create max_batch)", f.NB, c->max_batch);
    if (a.scale_by_sigma && !c->tiled) return fail("scale_by_sigma=True is only built for the tiled plan (the shipped GTO-Halo config sets it False, RD/configs/model/ncsnpp.yaml)");
    if (a.conditional && !f.labels) return fail("class_labels is required: the model is conditional (label_emb) -- reference raises here too (RD/models/ncsnpp.py:262)");
    const int T = c->temb, Np_t = (T + 63) & ~63, Np_d = (c->dense_total + 63) & ~63;
    // ---- embedding: Fourier -> Linear -> SiLU -> Linear (+label_emb) -> [SiLU -> all Dense_0]
    if (!f.tt_row && !f.dense_rows) {
    LinArgs l{};
    l.M = f.NB; l.fourW = P(c, "time_embed.W"); l.nfour = a.nf;
    l.X = f.sig; l.x_mod = f.sig_mod > 0 ? f.sig_mod : f.NB; l.t_is_time = f.t_is_time; l.smin = f.smin; l.ratio = f.ratio;
    l.use_scalar = f.sig ? 0 : 1; l.t_scalar = f.t_scalar;
    l.pre = 2; l.K = pad16(2 * a.nf); l.W = c->d_w.get() + c->w_t0; l.Npad = Np_t; l.N = T; l.bias = P(c, "time_mlp.0.bias");
    l.Y = c->d_h1.get(); l.ldy = T;
    {
        ProfScope ps(c, s, "linear_mfma(time_mlp.0)", 2.0 * f.NB * T * 2 * a.nf);
        hipLaunchKernelGGL(linear_mfma_kernel<1>, dim3((unsigned)ceil_div(f.NB, 16), (unsigned)(Np_t / 64)), dim3(RDMI_THREADS), 0, s, l);
    }
    LinArgs l2{};
    l2.M = f.NB; l2.X = c->d_h1.get(); l2.ldx = T; l2.pre = 1; l2.K = T; l2.W = c->d_w.get() + c->w_t2; l2.Npad = Np_t; l2.N = T;
    l2.bias = P(c, "time_mlp.2.bias"); l2.Y = c->d_temb.get(); l2.ldy = T;
    if (a.conditional) { l2.labels = f.labels; l2.Wl = P(c, "label_emb.weight"); l2.bl = P(c, "label_emb.bias"); l2.ncls = a.num_classes; l2.label_rows = f.label_rows; }
    {
        ProfScope ps(c, s, "linear_mfma(time_mlp.2)", 2.0 * f.NB * T * T);
        hipLaunchKernelGGL(linear_mfma_kernel<1>, dim3((unsigned)ceil_div(f.NB, 16), (unsigned)(Np_t / 64)), dim3(RDMI_THREADS), 0, s, l2);
    }
    }
    if (!f.dense_rows) {
    LinArgs l3{};
    l3.M = f.NB; l3.X = c->d_temb.get(); l3.ldx = T; l3.pre = 1; l3.K = T;
    if (f.tt_row) {     // every sample shares the time row; the label embedding is added in the prologue (same sums as time_mlp.2's epilogue)
        l3.X = f.tt_row; l3.ldx = 0; l3.pre = 3;
        if (a.conditional) { l3.labels = f.labels; l3.Wl = P(c, "label_emb.weight"); l3.ncls = a.num_classes; l3.label_rows = f.label_rows; }
    } l3.W = c->d_w.get() + c->w_dense; l3.Npad = Np_d; l3.N = c->dense_total;
    l3.bias = c->d_w.get() + c->b_dense; l3.Y = c->d_dense.get(); l3.ldy = c->dense_total;
    {
        ProfScope ps(c, s, "linear_mfma(Dense_0 x all)", 2.0 * f.NB * T * c->dense_total);
        hipLaunchKernelGGL((linear_mfma_kernel<1, 16>), dim3((unsigned)ceil_div(f.NB, 16), (unsigned)(Np_d / 64)), dim3(RDMI_THREADS), 0, s, l3);
    }
    }
    HIP_OK(hipGetLastError());
    if (a.compute_dtype == 1 && !c->tiled && !c->in_train_forward)
        return fail("compute_dtype=bf16 on this shape is built for the TRAINING step only (model.train_dtype = 'bf16'); sampling and evaluation of the "
                    "GTO-Halo model run the exact-fp32 plans");
    if (c->tiled) return run_tiled(c, f, s);
    // ---- the U-Net: one workgroup-resident launch (csrc/unet_kernel.h) ...
    const FusedProg* fq = (c->use_fused && !c->debug_taps && c->fused) ? c->fused->pick(f.NB) : nullptr;
    if (c->in_train_forward) {      // one sample per workgroup pays while the batch fits the chip in about one wave of workgroups; beyond that the layer plan (bf16 MFMA) is faster
        static const int fused_upto = [] { const char* e = std::getenv("RDMI_TRAIN_FUSED_UPTO"); return e ? atoi(e) : 2 * std::max(resident_workgroups(), 1); }();
        fq = (c->fused && f.NB <= fused_upto) ? c->fused->training() : nullptr;
    }
    if (fq) return run_fused(c, *fq, f, s);
    // ---- ... or the layer-by-layer plan (debug taps, shapes the fused planner cannot fit in LDS)
    for (auto& op : c->ops) {
        if (op.kind == OP_CONV) {
            ConvArgs ca = op.conv;
            ca.NB = f.NB;
            if (op.a_is_input) { ca.srcA = f.x; ca.srcA_mod = f.x_mod; }
            if (op.out_is_output) ca.out = f.out;
            if (op.use_dense && f.dense_rows) ca.dense = f.dense_rows;
            ProfScope ps(c, s, cfg_name(op.cfg), op.flops_per_sample * f.NB);
            if (int e = launch_conv(op.cfg, ca, s)) return e;
        } else {
            AttnArgs aa = op.attn;
            aa.NB = f.NB;
            ProfScope ps(c, s, "attn_mfma<64>", op.flops_per_sample * f.NB);
            if (int e = launch_attn(aa, s)) return e;
        }
    }
    return 0;
}

}  // namespace

#include "train_plan.h"
#include "tiled_train.h"

// The non-memory handles of a training plan, in this order; its buffers (and the tiled part) are released with the members after.
TrainPlan::~TrainPlan() {
    if (side) (void)hipStreamSynchronize(side);
    if (fwd_exec) (void)hipGraphExecDestroy(fwd_exec);
    for (auto& e : bwd_exec) if (e) (void)hipGraphExecDestroy(e);
    for (int p = 0; p < 2; ++p) {
        if (ev_ready[p]) (void)hipEventDestroy(ev_ready[p]);
        if (ev_done[p]) (void)hipEventDestroy(ev_done[p]);
    }
    if (side) (void)hipStreamDestroy(side);
    if (cap) (void)hipStreamDestroy(cap);
}

// the training plan first (it synchronises its side stream), then the profiling events; the buffers go with the members
rdmi_ctx::~rdmi_ctx() {
    train.reset();
    for (auto& ev : ev_pool) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
}

// ============================================================================================
// C ABI
// ============================================================================================
extern "C" {

const char* rdmi_last_error(void) { return g_err.c_str(); }
int rdmi_debug_op_cycles(rdmi_ctx* c, long long* host, int cap, const char** desc, int desc_cap) {
    if (!c || !fused_ready(c) || !c->fused->d_stamps) return 0;
    const long long* d_stamps = c->fused->d_stamps.get();
    const FusedProg& q0 = c->fused->progs[(size_t)std::min<int>(std::max(c->fused->last_prog, 0), (int)c->fused->progs.size() - 1)];     // the program of the last launch
    const int n = (int)q0.fprog.size();
    std::vector<long long> st((size_t)n + 1);
    if (n > 1000) return 0;
    if (hipMemcpy(st.data(), d_stamps, st.size() * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    for (int i = 0; i < n && i < cap; ++i) host[i] = st[(size_t)i + 1] - st[(size_t)i];
    // fine stamps of CONV ops (entry, ring issued, first B landed, main done, shortcut done, epilogue done) follow at cap/2
    {
        std::vector<long long> fs((size_t)n * 8);
        if (hipMemcpy(fs.data(), d_stamps + 1024, fs.size() * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess)
            for (int i = 0; i < n && 256 + i * 8 + 7 < cap; ++i)
                for (int k = 0; k < 8; ++k) host[256 + i * 8 + k] = fs[(size_t)i * 8 + k] - st[(size_t)i];
    }
    for (int i = 0; i < n && i < desc_cap; ++i) desc[i] = q0.fdesc[(size_t)i].c_str();
    return n;
}

int rdmi_debug_program(rdmi_ctx* c, int prog, int* S, int* coop, int* train, const char** desc, int desc_cap) {
    if (!c || !c->fused || prog < 0 || prog >= (int)c->fused->progs.size() || !c->fused->progs[(size_t)prog].ok) return -1;
    const FusedProg& q = c->fused->progs[(size_t)prog];
    if (S) *S = q.S;
    if (coop) *coop = q.coop ? 1 : 0;
    if (train) *train = q.train ? 1 : 0;
    const int n = (int)q.fdesc.size();
    for (int i = 0; desc && i < n && i < desc_cap; ++i) desc[i] = q.fdesc[(size_t)i].c_str();
    return n;
}

int rdmi_debug_packed(rdmi_ctx* c, const char* key, float* dst, size_t numel, void* stream) {
    if (!c || !key || !dst) return fail("null argument");
    auto it = c->wmap.find(key);
    if (it == c->wmap.end()) return fail("no packed tensor '%s'", key);
    if (it->second + numel > c->w_floats) return fail("packed tensor '%s': %zu floats exceed the arena", key, numel);
    HIP_OK(hipMemcpyAsync(dst, c->d_w.get() + it->second, numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

const char* rdmi_path_info(rdmi_ctx* c) {
    static thread_local std::string s;
    if (!c) return "";
    if (c->tiled) {
        s = std::string("tiled (") + (c->arch.compute_dtype == 1 ? "bf16 MFMA operands, fp32 accumulate" : "fp32") + "): " + std::to_string(c->tiled->launches.size()) + " launches over HBM-resident NHWC tensors (" + std::to_string(c->tiled->ws_per_sample * 4 / 1024) + " KiB of activations per sample)";
        long n_resize = 0;
        for (auto& l : c->tiled->launches) n_resize += std::holds_alternative<TResizeL>(l.op);
        s += "; resize launches (h onto an odd skip grid): " + std::to_string(n_resize);
    } else {
        const std::vector<FusedProg>& progs = c->fused->progs;      // every context that does not run the tiled plan has a FusedPlan
        if (fused_ready(c) && c->use_fused && !c->debug_taps) {
            s = "fused: workgroup-resident U-Net, " + std::to_string(progs[0].fprog.size()) + " ops, " + std::to_string(progs[0].fused_lds) + " B LDS";
            for (size_t i = 1; i < progs.size(); ++i)
                if (progs[i].coop)
                    s += progs[i].ok ? "; co-operative groups of 4 workgroups up to batch " + std::to_string(progs[i].max_nb) + " (" + std::to_string(progs[i].fprog.size()) + " ops, " + std::to_string(progs[i].n_xchg) + " exchanges, id stride " + std::to_string(c->fused->coop_stride) + (c->fused->use_coop ? ")" : ", disabled)")
                                        : "; co-operative program unavailable (" + progs[i].why + ")";
                else
                s += progs[i].ok ? "; S=" + std::to_string(progs[i].S) + " samples/workgroup from batch " + std::to_string(c->fused->s_min_wg * progs[i].S) + " (" + std::to_string(progs[i].fprog.size()) + " ops)"
                                    : "; S=" + std::to_string(progs[i].S) + " unavailable (" + progs[i].why + ")";
        } else {
            s = "layers: " + std::to_string(c->ops.size()) + " launches" + (fused_ready(c) ? "" : " (fused unavailable: " + (progs.empty() ? std::string("not built") : progs[0].why) + ")");
        }
        for (auto& q : progs) if (q.train && !q.ok) s += "; fused training forward unavailable (" + q.why + ")";
        if (c->fused->training())
            s += "; training forward: fused program (" + std::to_string(c->fused->training()->fprog.size()) + " ops, layer outputs stashed for the backward)";
    }
    if (c->train) s += "; input-gradient backward calls: " + std::to_string(c->train->input_dgrad_calls);
    return s.c_str();
}

int rdmi_philox_normal(float* z, size_t n, unsigned long long seed, unsigned long long elem_offset, unsigned draw, void* stream) {
    if (n == 0) return 0;
    if (!z) return fail("null argument");
    hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)((n + 4 * RDMI_THREADS - 1) / (4 * RDMI_THREADS))), dim3(RDMI_THREADS), 0, (hipStream_t)stream, z, (long)n,
                       (uint64_t)seed, (uint64_t)elem_offset, (const int*)nullptr, (int)draw);
    HIP_OK(hipGetLastError());
    return 0;
}

// 0: no co-operative exchange of this context has ever given up its bounded wait; 1: one did (the affected output samples are NaN).
// Synchronises the device (diagnostic: tests and bench.py call it after their timed regions).
int rdmi_coop_status(rdmi_ctx* c, int* gave_up) {
    if (!c || !gave_up) return fail("null argument");
    *gave_up = 0;
    if (!c->fused) return 0;
    for (auto& q : c->fused->progs)
        if (q.coop && q.d_coop_err) { int v = 0; HIP_OK(hipMemcpy(&v, q.d_coop_err.get(), sizeof v, hipMemcpyDeviceToHost)); *gave_up |= v; }
    if (*gave_up) c->fused->use_coop = false;       // the groups of this device were not co-resident once: later calls take the single-sample programs
    return 0;
}
const char* rdmi_version(void) {
#ifdef RDMI_EMU
    return "rdmi 0.1 (CPU execution-model emulator build: tests only)";
#else
    return "rdmi 0.1 (gfx950)";
#endif
}

int rdmi_create(const rdmi_arch* arch, int max_batch, int H, int W, rdmi_ctx** out) {
    if (!arch || !out) return fail("null argument");
    if (arch->n_levels < 1 || arch->n_levels > RDMI_MAX_LEVELS) return fail("n_levels=%d out of range", arch->n_levels);
    if (arch->nf % 16 != 0) return fail("nf=%d must be a multiple of 16", arch->nf);
    if (max_batch < 1 || H < 2 || W < 2) return fail("bad shape max_batch=%d H=%d W=%d", max_batch, H, W);
    rdmi_ctx* c = new rdmi_ctx();
    c->arch = *arch;
    c->max_batch = max_batch; c->H = H; c->W = W;
    c->temb = arch->nf * 4;
    if (const char* e = std::getenv("RDMI_DEBUG_TAPS")) c->debug_taps = atoi(e) != 0;
    if (const char* e = std::getenv("RDMI_PATH")) c->use_fused = std::string(e) != "layers";
    int e = 0;
    try { e = build_plan(c); } catch (const std::exception& ex) { e = fail("plan construction failed: %s", ex.what()); }
    if (e) { delete c; return e; }
    *out = c;
    return 0;
}

int rdmi_destroy(rdmi_ctx* c) {
    delete c;
    return 0;
}

int rdmi_num_params(const rdmi_ctx* c) { return c ? (int)c->params.size() : 0; }

int rdmi_param_info(const rdmi_ctx* c, int index, const char** name, size_t* numel) {
    if (!c || index < 0 || index >= (int)c->params.size()) return fail("param index %d out of range", index);
    if (name) *name = c->params[(size_t)index].name.c_str();
    if (numel) *numel = c->params[(size_t)index].numel;
    return 0;
}

int rdmi_set_param(rdmi_ctx* c, const char* name, const float* dev_ptr, size_t numel) {
    if (!c || !name || !dev_ptr) return fail("null argument");
    auto it = c->pindex.find(name);
    if (it == c->pindex.end()) return fail("unknown parameter '%s'", name);
    Param& p = c->params[(size_t)it->second];
    if (p.numel != numel) return fail("parameter '%s': expected %zu elements, got %zu", name, p.numel, numel);
    if (p.ptr != dev_ptr) c->packed_valid = false;
    p.ptr = dev_ptr;
    return 0;
}

int rdmi_repack(rdmi_ctx* c, void* stream) {
    if (!c) return fail("null context");
    return do_repack(c, (hipStream_t)stream);
}

static int maybe_repack(rdmi_ctx* c, unsigned flags, hipStream_t s) {
    if ((flags & RDMI_PARAMS_CACHED) && c->packed_valid) return 0;
    return do_repack(c, s);
}

int rdmi_forward(rdmi_ctx* c, const float* x, const float* sigma, const float* labels, float* out, int B,
                 unsigned flags, void* stream) {
    if (!c || !x || !sigma || !out) return fail("null argument");
    hipStream_t s = (hipStream_t)stream;
    if (int e = maybe_repack(c, flags, s)) return e;
    FwdIn f{x, 0, sigma, 0, 0.f, 0, 0.f, 0.f, labels, B, out, B};
    int e = run_forward(c, f, s);
    if (c->profiling) prof_collect(c);
    return e;
}

int rdmi_score(rdmi_ctx* c, const float* x, const float* t, const float* labels, float* out, int B,
               double sigma_min, double sigma_max, unsigned flags, void* stream) {
    if (!c || !x || !t || !out) return fail("null argument");
    hipStream_t s = (hipStream_t)stream;
    if (int e = maybe_repack(c, flags, s)) return e;
    FwdIn f{x, 0, t, 0, 0.f, 1, (float)sigma_min, (float)(sigma_max / sigma_min), labels, B, out, B};
    int e = run_forward(c, f, s);
    if (c->profiling) prof_collect(c);
    return e;
}

static int cf_score_impl(rdmi_ctx* c, const float* x, const float* t, int t_mod, const float* labels, const float* weight,
                         float* out, int B, float smin, float ratio, hipStream_t s) {
    const int E = c->H * c->W * c->arch.channels;
    FwdIn f{x, B, t, t_mod, 0.f, 1, smin, ratio, labels, B, c->d_s2.get(), 2 * B};
    if (int e = run_forward(c, f, s)) return e;
    {
        ProfScope ps(c, s, "cfg_combine", 0);
        hipLaunchKernelGGL(cfg_combine_kernel, dim3((unsigned)ceil_div(B * E, RDMI_THREADS)), dim3(RDMI_THREADS), 0, s,
                           (const float*)c->d_s2.get(), weight, out, B, E);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

int rdmi_cf_score(rdmi_ctx* c, const float* x, const float* t, const float* labels, const float* weight, float* out,
                  int B, double sigma_min, double sigma_max, unsigned flags, void* stream) {
    if (!c || !x || !t || !labels || !out) return fail("null argument");
    if (2 * B > c->max_batch) return fail("CFG needs a model batch of 2*B=%d > max_batch=%d", 2 * B, c->max_batch);
    hipStream_t s = (hipStream_t)stream;
    if (int e = maybe_repack(c, flags, s)) return e;
    int e = cf_score_impl(c, x, t, B, labels, weight, out, B, (float)sigma_min, (float)(sigma_max / sigma_min), s);
    if (c->profiling) prof_collect(c);
    return e;
}

int rdmi_reflect(const float* in, float* out, size_t n, void* stream) {
    if (!in || !out) return fail("null argument");
    hipLaunchKernelGGL(reflect_kernel, dim3((unsigned)((n + RDMI_THREADS - 1) / RDMI_THREADS)), dim3(RDMI_THREADS), 0,
                       (hipStream_t)stream, in, out, (long)n);
    HIP_OK(hipGetLastError());
    return 0;
}

int rdmi_score_hk(const float* x, const float* x_orig, const float* sigma, float* out, int B, int E, int efs, int refls,
                  float min_cutoff, void* stream) {
    if (!x || !x_orig || !sigma || !out) return fail("null argument");
    hipLaunchKernelGGL(score_hk_kernel, dim3((unsigned)ceil_div(B * E, RDMI_THREADS)), dim3(RDMI_THREADS), 0, (hipStream_t)stream,
                       x, x_orig, sigma, out, B, E, efs, refls, min_cutoff);
    HIP_OK(hipGetLastError());
    return 0;
}


static float g_const(double smin, double smax) {
    // torch.sqrt(torch.tensor(2 * (np.log(sigma_max) - np.log(sigma_min)), dtype=float32))   RD/sde_lib.py:138-139
    return sqrtf((float)(2.0 * (std::log(smax) - std::log(smin))));
}

int rdmi_perturb(const float* batch, const float* z, const float* t, float* out, int B, int E, double sigma_min,
                 double sigma_max, void* stream) {
    if (!batch || !z || !t || !out) return fail("null argument");
    hipLaunchKernelGGL(perturb_kernel, dim3((unsigned)ceil_div(B * E, RDMI_THREADS)), dim3(RDMI_THREADS), 0, (hipStream_t)stream, batch,
                       z, t, out, B, E, (float)sigma_min, (float)(sigma_max / sigma_min));
    HIP_OK(hipGetLastError());
    return 0;
}

int rdmi_gto_pack(const float* data, const long long* idx, float* images, float* labels, int B, int row_len, int elems, double mean,
                  double std, void* stream) {
    if (B == 0) return 0;
    if (!data || !images || !labels) return fail("null argument");
    if (B < 0 || row_len < 1 || elems < row_len) return fail("gto_pack: rows of %d values into images of %d", row_len, elems);
    hipLaunchKernelGGL(gto_pack_kernel, dim3((unsigned)ceil_div(B * elems, RDMI_THREADS)), dim3(RDMI_THREADS), 0, (hipStream_t)stream, data, idx, images,
                       labels, B, row_len, elems, (float)mean, (float)std);
    HIP_OK(hipGetLastError());
    return 0;
}

int rdmi_gto_unnormalize(const float* samples, float* out, unsigned long long* clip_count, int N, int row_elems, void* stream) {
    if (N == 0) return 0;
    if (!samples || !out) return fail("null argument");
    if (N < 0 || row_elems < 67) return fail("gto_unnormalize: rows of %d values (need >= 67)", row_elems);
    hipLaunchKernelGGL(gto_unnormalize_kernel, dim3((unsigned)ceil_div(N * 22, RDMI_THREADS)), dim3(RDMI_THREADS), 0, (hipStream_t)stream, samples, out,
                       clip_count, N, row_elems);
    HIP_OK(hipGetLastError());
    return 0;
}

int rdmi_sm_loss(const float* score, const float* perturbed, const float* batch, const float* t, float* per_sample,
                 float* dscore, int B, int E, double sigma_min, double sigma_max, int likelihood_weighting, int reduce_mean,
                 void* stream) {
    if (!score || !perturbed || !batch || !t || !per_sample) return fail("null argument");
    hipLaunchKernelGGL(sm_loss_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, score, perturbed, batch, t, per_sample, dscore, B, E,
                       (float)sigma_min, (float)(sigma_max / sigma_min), g_const(sigma_min, sigma_max), likelihood_weighting, reduce_mean,
                       20, 10, 1e-2f);
    HIP_OK(hipGetLastError());
    return 0;
}

int rdmi_em_update(const float* x, const float* score, const float* z, const float* t, float* x_out, float* x_mean_out,
                   int B, int E, int N, double sigma_min, double sigma_max, void* stream) {
    if (!x || !score || !z || !t || !x_out) return fail("null argument");
    hipLaunchKernelGGL(em_update_kernel, dim3((unsigned)ceil_div(B * E, RDMI_THREADS)), dim3(RDMI_THREADS), 0,
                       (hipStream_t)stream, x, score, z, t, (const float*)nullptr, (const StepState*)nullptr, x_out,
                       x_mean_out, (float*)nullptr, B, E, N, (float)sigma_min, (float)(sigma_max / sigma_min),
                       g_const(sigma_min, sigma_max), 0);
    HIP_OK(hipGetLastError());
    return 0;
}

int rdmi_pf_drift_div(const float* score, const float* gx, const float* eps, const float* t, float* drift, float* div, int B, int E,
                      double sigma_min, double sigma_max, void* stream) {
    if (!score || !gx || !eps || !t || !drift || !div) return fail("null argument");
    if (B < 1 || E < 1) return fail("pf_drift_div: %d samples of %d elements", B, E);
    hipLaunchKernelGGL(pf_drift_div_kernel, dim3((unsigned)B), dim3(RDMI_THREADS), 0, (hipStream_t)stream, score, gx, eps, t, drift, div, E, sigma_min,
                       sigma_max / sigma_min, 2.0 * (std::log(sigma_max) - std::log(sigma_min)));
    HIP_OK(hipGetLastError());
    return 0;
}

int rdmi_langevin_update(const float* x, const float* score, const float* z, float* x_out, float* x_mean_out,
                         float* scratch, int B, int E, float snr, void* stream) {
    if (!x || !score || !z || !x_out || !scratch) return fail("null argument");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)B), dim3(64), 0, s, score, z, (const StepState*)nullptr, scratch, B, E, 0);
    hipLaunchKernelGGL(langevin_update_kernel, dim3((unsigned)ceil_div(B * E, RDMI_THREADS)), dim3(RDMI_THREADS), 64, s, x,
                       score, z, (const float*)scratch, (const StepState*)nullptr, x_out, x_mean_out, B, E, snr, 0);
    HIP_OK(hipGetLastError());
    return 0;
}

int rdmi_pc_sample(rdmi_ctx* c, float* x, const float* labels, const float* weight, const float* noise, float* trace,
                   const float* teacher, int B, const rdmi_pc_opts* o, unsigned flags, void* stream) {
    if (!c || !x || !o) return fail("null argument");
    if (o->N < 2) return fail("N=%d: need at least 2 scales", o->N);
    if (o->corrector != 0 && o->corrector != 1) return fail("unknown corrector id %d", o->corrector);
    const int NBm = o->use_cfg ? 2 * B : B;
    if (NBm > c->max_batch) return fail("model batch %d > max_batch=%d", NBm, c->max_batch);
    if (o->use_cfg && !labels) return fail("use_cfg=1 needs class_labels");
    hipStream_t s = (hipStream_t)stream;
    if (int e = maybe_repack(c, flags, s)) return e;
    const int E = c->H * c->W * c->arch.channels;
    const long BE = (long)B * E;
    const float smin = (float)o->sigma_min, ratio = (float)(o->sigma_max / o->sigma_min);
    const float gc = g_const(o->sigma_min, o->sigma_max);
    const unsigned gBE = (unsigned)ceil_div((int)BE, RDMI_THREADS);
    const uint64_t eoff = (uint64_t)o->seq_offset * (uint64_t)E;

    // timesteps = torch.linspace(T=1, eps, N): fp32 step, fma(step, i, start) / fma(-step, N-1-i, end)
    std::vector<float> ts((size_t)o->N);
    {
        const float start = 1.0f, end = o->eps;
        const double step = (double)(float)((end - start) / (float)(o->N - 1));
        for (int i = 0; i < o->N; ++i)
            ts[(size_t)i] = (float)(i < o->N / 2 ? (double)start + step * i : (double)end - step * (o->N - 1 - i));
    }
    // The time path of the embedding (Fourier -> time_mlp.0 -> SiLU -> time_mlp.2, + both biases) depends only on the
    // update's t, which is known up front: evaluate it for ALL updates in two launches (one row per update) instead of two
    // launches per score evaluation; per evaluation only the batched Dense_0 GEMM remains, which adds the label embedding
    // to the shared row in its prologue.
    const int nupd = o->N - 1, T = c->temb, Np_t = (T + 63) & ~63, Np_d = (c->dense_total + 63) & ~63;
    if (c->tt_cap < nupd) {
        c->d_tt.reset(); c->d_th1.reset(); c->d_ts.reset(); c->tt_cap = 0;
        HIP_OK(hip_alloc(c->d_tt, (size_t)pad16(nupd) * T));
        HIP_OK(hip_alloc(c->d_th1, (size_t)pad16(nupd) * T));
        HIP_OK(hip_alloc(c->d_ts, (size_t)pad16(nupd)));
        c->tt_cap = nupd;
    }
    const rdmi_arch& a = c->arch;
    {
        // the time grid is formed on the device by the same double-precision expression as the host copy above (no host
        // buffer has to outlive this call: every rdmi entry point is asynchronous on `stream`)
        hipLaunchKernelGGL(linspace_kernel, dim3((unsigned)ceil_div(nupd, RDMI_THREADS)), dim3(RDMI_THREADS), 0, s, c->d_ts.get(), nupd, o->N, 1.0f, o->eps);
        LinArgs l{};
        l.M = nupd; l.fourW = P(c, "time_embed.W"); l.nfour = a.nf; l.X = c->d_ts.get(); l.x_mod = nupd; l.t_is_time = 1; l.smin = smin; l.ratio = ratio;
        l.pre = 2; l.K = pad16(2 * a.nf); l.W = c->d_w.get() + c->w_t0; l.Npad = Np_t; l.N = T; l.bias = P(c, "time_mlp.0.bias"); l.Y = c->d_th1.get(); l.ldy = T;
        LinArgs l2{};
        l2.M = nupd; l2.X = c->d_th1.get(); l2.ldx = T; l2.pre = 1; l2.K = T; l2.W = c->d_w.get() + c->w_t2; l2.Npad = Np_t; l2.N = T;
        l2.bias = P(c, "time_mlp.2.bias"); l2.Y = c->d_tt.get(); l2.ldy = T;
        if (a.conditional) l2.bl = P(c, "label_emb.bias");
        ProfScope ps(c, s, "linear_mfma(time path, all updates)", 2.0 * nupd * T * (2 * a.nf + T));
        hipLaunchKernelGGL(linear_mfma_kernel<1>, dim3((unsigned)ceil_div(nupd, 16), (unsigned)(Np_t / 64)), dim3(RDMI_THREADS), 0, s, l);
        hipLaunchKernelGGL(linear_mfma_kernel<1>, dim3((unsigned)ceil_div(nupd, 16), (unsigned)(Np_t / 64)), dim3(RDMI_THREADS), 0, s, l2);
        HIP_OK(hipGetLastError());
    }
    // Dense_0 (the 17 per-block projections of SiLU(temb), RD/models/layerspp.py:202) depends on (update, sample) only through
    // the update's time row and the sample's label: it is evaluated for a whole CHUNK of updates in one GEMM launch
    // ([U * NBm] rows: a real dense contraction instead of 999 launches of 256 rows) into a buffer of at most ~256 MB;
    // row (u, n) = Dense_0(SiLU(tt[u] + label_emb(labels[n]))): the same sums in the same order as the stand-alone path.
    const size_t dense_row_floats = (size_t)NBm * c->dense_total;
    const int U = (int)std::max<size_t>(1, std::min<size_t>((size_t)nupd, ((size_t)256 << 20) / (dense_row_floats * sizeof(float))));
    if (c->dense_all_cap < (size_t)U * dense_row_floats) {
        c->dense_all_cap = 0;
        HIP_OK(hip_alloc(c->d_dense_all, (size_t)U * dense_row_floats));
        c->dense_all_cap = (size_t)U * dense_row_floats;
    }
    auto dense_chunk = [&](int i0) -> int {
        const int u = std::min(U, nupd - i0);
        LinArgs l3{};
        l3.M = u * NBm; l3.X = c->d_tt.get() + (size_t)i0 * T; l3.ldx = T; l3.pre = 3; l3.K = T; l3.row_div = NBm;
        if (a.conditional && labels) { l3.labels = labels; l3.Wl = P(c, "label_emb.weight"); l3.ncls = a.num_classes; l3.label_rows = B; }
        l3.W = c->d_w.get() + c->w_dense; l3.Npad = Np_d; l3.N = c->dense_total;
        l3.bias = c->d_w.get() + c->b_dense; l3.Y = c->d_dense_all.get(); l3.ldy = c->dense_total;
        ProfScope ps(c, s, "linear_mfma(Dense_0 x all, chunk of updates)", 2.0 * l3.M * T * c->dense_total);
        hipLaunchKernelGGL((linear_mfma_kernel<1, 16>), dim3((unsigned)ceil_div(l3.M, 16), (unsigned)(Np_d / 64)), dim3(RDMI_THREADS), 0, s, l3);
        HIP_OK(hipGetLastError());
        return 0;
    };
    // one score evaluation at update i's shared time: the raw network output lands in d_s2 ([2B] with CFG, [B] without)
    auto net_eval = [&](int i, float t) -> int {
        FwdIn f{x, o->use_cfg ? B : 0, nullptr, 0, t, 1, smin, ratio, labels, B, c->d_s2.get(), NBm};
        f.tt_row = c->d_tt.get() + (size_t)i * T;
        f.dense_rows = c->d_dense_all.get() + (size_t)(i % U) * dense_row_floats;
        return run_forward(c, f, s);
    };
    uint32_t draw = 0;
    for (int i = 0; i < o->N - 1; ++i) {
        const float t = ts[(size_t)i];
        if (i % U == 0) { if (int e = dense_chunk(i)) return e; }
        if (o->corrector == 1) {
            for (int k = 0; k < o->n_steps_each; ++k, ++draw) {
                if (int e = net_eval(i, t)) return e;
                ProfScope ps(c, s, "langevin_update", 0);
                hipLaunchKernelGGL(langevin_prep_kernel, dim3((unsigned)B), dim3(64), 0, s, (const float*)c->d_s2.get(), weight,
                                   noise ? noise + (size_t)draw * BE : (const float*)nullptr, c->d_score.get(), c->d_z.get(), c->d_norms.get(), B, E,
                                   o->use_cfg, (uint64_t)o->seed, eoff, draw);
                hipLaunchKernelGGL(langevin_update_kernel, dim3(gBE), dim3(RDMI_THREADS), 64, s, (const float*)x,
                                   (const float*)c->d_score.get(), (const float*)c->d_z.get(), (const float*)c->d_norms.get(), (const StepState*)nullptr, x,
                                   (float*)nullptr, B, E, o->snr, 0);
            }
        }
        if (int e = net_eval(i, t)) return e;
        {
            ProfScope ps(c, s, "em_fused", 0);
            hipLaunchKernelGGL(em_fused_kernel, dim3(gBE), dim3(RDMI_THREADS), 0, s, (const float*)x, (const float*)c->d_s2.get(), weight,
                               noise ? noise + (size_t)draw * BE : (const float*)nullptr, x, trace ? trace + (size_t)i * BE : (float*)nullptr,
                               teacher ? teacher + (size_t)i * BE : (const float*)nullptr, B, E, o->N, t, smin, ratio, gc, o->use_cfg,
                               (uint64_t)o->seed, eoff, draw);
            ++draw;
        }
        HIP_OK(hipGetLastError());
        if (c->profiling && (i % 16 == 15)) prof_collect(c);
    }
    if (c->profiling) prof_collect(c);
    return 0;
}

// ---- probability-flow ODE sampler: scipy's RK45 (Dormand-Prince 5(4), scipy/integrate/_ivp/rk.py) with the state on the device ----
int rdmi_ode_sample(rdmi_ctx* c, float* x, const float* labels, const float* weight, int B, const rdmi_ode_opts* o, int* nfev_out,
                    double* t_final, unsigned flags, void* stream) {
    if (!c || !x || !o) return fail("null argument");
    const int NBm = o->use_cfg ? 2 * B : B;
    if (NBm > c->max_batch) return fail("model batch %d > max_batch=%d", NBm, c->max_batch);
    if (o->use_cfg && !labels) return fail("use_cfg=1 needs class_labels");
    if (!(o->rtol > 0) || !(o->atol > 0)) return fail("rtol / atol must be positive");
    hipStream_t s = (hipStream_t)stream;
    if (int e = maybe_repack(c, flags, s)) return e;
    const int E = c->H * c->W * c->arch.channels;
    const long n = (long)B * E;
    const unsigned gn = (unsigned)ceil_div((int)n, RDMI_THREADS);
    const float smin = (float)o->sigma_min, ratio = (float)(o->sigma_max / o->sigma_min), gc = g_const(o->sigma_min, o->sigma_max);
    // Dormand-Prince tableau as scipy holds it (rk.py: class RK45)
    static const double Cc[6] = {0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1};
    static const double A[6][5] = {{0, 0, 0, 0, 0}, {1.0 / 5, 0, 0, 0, 0}, {3.0 / 40, 9.0 / 40, 0, 0, 0}, {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
                                   {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
                                   {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
    static const double Bc[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
    static const double Ec[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
    const double SAFETY = 0.9, MIN_FACTOR = 0.2, MAX_FACTOR = 10, err_exp = -1.0 / 5;
    dev_ptr<double> y, ynew, Kd, f1, red;       // y / ynew swap on every accepted step
    dev_ptr<float> x32;
    HIP_OK(hip_alloc(y, (size_t)n));
    HIP_OK(hip_alloc(ynew, (size_t)n));
    HIP_OK(hip_alloc(Kd, 7 * (size_t)n));
    HIP_OK(hip_alloc(f1, (size_t)n));
    HIP_OK(hip_alloc(red, 4));
    HIP_OK(hip_alloc(x32, (size_t)n));
    double* const d_K = Kd.get(); double* const d_f1 = f1.get(); double* const d_red = red.get(); float* const d_x32 = x32.get();
    int nfev = 0;
    // fun(t, x32) -> Kout (float64 copy of the float32 drift * bump)
    auto fun = [&](double t, double* Kout) -> int {
        FwdIn f{d_x32, o->use_cfg ? B : 0, nullptr, 0, (float)t, 1, smin, ratio, labels, B, c->d_s2.get(), NBm};     // vec_t = ones(B) * t  (float32)
        if (int e = run_forward(c, f, s)) return e;
        hipLaunchKernelGGL(ode_rhs_kernel, dim3(gn), dim3(RDMI_THREADS), 0, s, (const float*)c->d_s2.get(), weight, (const float*)d_x32, Kout, B, E, (float)t, smin, ratio, gc,
                           o->use_cfg, o->moll);
        ++nfev;
        return 0;
    };
    auto norm_of = [&](int mode, const double* a, const double* b, const double* y0, double h, double* out_host) -> int {
        OdeNormArgs q{a, b, y0, d_K, n, mode, o->atol, o->rtol, h, {Ec[0], Ec[1], Ec[2], Ec[3], Ec[4], Ec[5], Ec[6]}, d_red, 0};
        hipLaunchKernelGGL(ode_norm_kernel, dim3(1), dim3(RDMI_THREADS), RDMI_THREADS * sizeof(double), s, q);
        double ss = 0;
        if (hipMemcpyAsync(&ss, d_red, sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return fail("ode: read-back failed");
        *out_host = std::sqrt(ss) / std::sqrt((double)n);            // scipy: norm(x) = ||x|| / sqrt(x.size)
        return 0;
    };
    const double t0 = o->T, t_bound = o->eps, direction = t_bound >= t0 ? 1.0 : -1.0;
    double t = t0;
    int rc = 0;
    hipLaunchKernelGGL(ode_f2d_kernel, dim3(gn), dim3(RDMI_THREADS), 0, s, (const float*)x, y.get(), n);
    hipLaunchKernelGGL(ode_stage_kernel, dim3(gn), dim3(RDMI_THREADS), 0, s, (const double*)y.get(), (const double*)d_K, n, 0, 0., 0., 0., 0., 0., 0., 0., (double*)nullptr, d_x32);
    if ((rc = fun(t, d_K))) return rc;                // self.f = fun(t0, y0)
    double h_abs;
    if (o->first_step > 0) h_abs = o->first_step;
    else {   // select_initial_step (scipy/integrate/_ivp/common.py), order = 4
        const double interval = std::fabs(t_bound - t0);
        double d0 = 0, d1 = 0, d2 = 0;
        if ((rc = norm_of(0, y.get(), nullptr, y.get(), 0, &d0)) || (rc = norm_of(0, d_K, nullptr, y.get(), 0, &d1))) return rc;
        double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        h0 = std::min(h0, interval);
        hipLaunchKernelGGL(ode_axpy_kernel, dim3(gn), dim3(RDMI_THREADS), 0, s, (const double*)y.get(), (const double*)d_K, h0 * direction, n, d_x32);
        if ((rc = fun(t0 + h0 * direction, d_f1))) return rc;
        if ((rc = norm_of(1, d_f1, d_K, y.get(), 0, &d2))) return rc;
        d2 /= h0;
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? std::max(1e-6, h0 * 1e-3) : std::pow(0.01 / std::max(d1, d2), 1.0 / 5);
        h_abs = std::min(std::min(100 * h0, h1), interval);
    }
    int steps = 0;
    while (direction * (t - t_bound) < 0) {
        if (o->max_steps > 0 && steps >= o->max_steps) break;
        const double min_step = 10 * std::fabs(std::nextafter(t, direction * INFINITY) - t);
        if (h_abs < min_step) h_abs = min_step;
        bool accepted = false, rejected = false;
        double t_new = t, h = 0;
        while (!accepted) {
            if (h_abs < min_step) return fail("ode: required step size is less than spacing between numbers (scipy: TOO_SMALL_STEP) at t=%g", t);
            h = h_abs * direction;
            t_new = t + h;
            if (direction * (t_new - t_bound) > 0) t_new = t_bound;
            h = t_new - t;
            h_abs = std::fabs(h);
            for (int st = 1; st < 6; ++st) {                         // rk_step: K[s] = fun(t + c_s h, y + h * K[:s].T a_s[:s])
                hipLaunchKernelGGL(ode_stage_kernel, dim3(gn), dim3(RDMI_THREADS), 0, s, (const double*)y.get(), (const double*)d_K, n, st, A[st][0], A[st][1], A[st][2], A[st][3],
                                   A[st][4], 0., h, (double*)nullptr, d_x32);
                if ((rc = fun(t + Cc[st] * h, d_K + (size_t)st * n))) return rc;
            }
            hipLaunchKernelGGL(ode_stage_kernel, dim3(gn), dim3(RDMI_THREADS), 0, s, (const double*)y.get(), (const double*)d_K, n, 6, Bc[0], Bc[1], Bc[2], Bc[3], Bc[4], Bc[5], h,
                               ynew.get(), d_x32);                       // y_new = y + h * K[:-1].T B
            if ((rc = fun(t + h, d_K + (size_t)6 * n))) return rc;      // f_new -> K[-1]
            double err = 0;
            if ((rc = norm_of(2, nullptr, ynew.get(), y.get(), h, &err))) return rc;
            if (err < 1) {
                double factor = err == 0 ? MAX_FACTOR : std::min(MAX_FACTOR, SAFETY * std::pow(err, err_exp));
                if (rejected) factor = std::min(1.0, factor);
                h_abs *= factor;
                accepted = true;
            } else {
                h_abs *= std::max(MIN_FACTOR, SAFETY * std::pow(err, err_exp));
                rejected = true;
            }
        }
        // accept: y <- y_new, f <- f_new (K[0] <- K[6])
        std::swap(y, ynew);
        HIP_OK(hipMemcpyAsync(d_K, d_K + (size_t)6 * n, n * sizeof(double), hipMemcpyDeviceToDevice, s));
        t = t_new;
        ++steps;
    }
    hipLaunchKernelGGL(ode_d2f_kernel, dim3(gn), dim3(RDMI_THREADS), 0, s, (const double*)y.get(), x, n);
    HIP_OK(hipStreamSynchronize(s));
    if (nfev_out) *nfev_out = nfev;
    if (t_final) *t_final = t;
    if (o->h_next_out) *o->h_next_out = h_abs;
    if (c->profiling) prof_collect(c);
    return 0;
}

// ---- multi-tensor optimizer (clip + Adam/AdamW + EMA), csrc/opt_kernels.h ---------------------------------------------
struct rdmi_opt {
    std::vector<OptSlot> h_slots;           // host mirror of the slot table (rdmi_opt_update_slots uploads from here)
    int nslots = 0, nchunks = 0;
    dev_ptr<OptSlot> d_slots; dev_ptr<OptChunk> d_chunks; dev_ptr<int> d_first; dev_ptr<float> d_partial, d_norm;
};

int rdmi_opt_create(const rdmi_opt_slot* slots, int n, rdmi_opt** out) {
    if (!slots || !out || n < 1) return fail("rdmi_opt_create: null / empty slot table");
    static_assert(sizeof(rdmi_opt_slot) == sizeof(OptSlot), "ABI slot layout");
    std::vector<OptChunk> chunks;
    std::vector<int> first((size_t)n + 1);
    for (int t = 0; t < n; ++t) {
        if (!slots[t].param || !slots[t].grad || !slots[t].exp_avg || !slots[t].exp_avg_sq) return fail("rdmi_opt_create: slot %d has a null pointer", t);
        if (slots[t].numel >= (1ull << 32)) return fail("rdmi_opt_create: slot %d has %llu elements (>= 2^32)", t, slots[t].numel);
        first[(size_t)t] = (int)chunks.size();
        for (unsigned long long o = 0; o < slots[t].numel; o += OPT_CHUNK) chunks.push_back({t, (unsigned)o});
    }
    first[(size_t)n] = (int)chunks.size();
    auto q = std::make_unique<rdmi_opt>();
    q->nslots = n; q->nchunks = (int)chunks.size();
    HIP_OK(hip_alloc(q->d_slots, (size_t)n));
    HIP_OK(hip_alloc(q->d_chunks, std::max<size_t>(chunks.size(), 1)));
    HIP_OK(hip_alloc(q->d_first, (size_t)n + 1));
    HIP_OK(hip_alloc(q->d_partial, std::max<size_t>(chunks.size(), 1)));
    HIP_OK(hip_alloc(q->d_norm, 2));
    HIP_OK(hipMemcpy(q->d_slots.get(), slots, (size_t)n * sizeof(OptSlot), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(q->d_chunks.get(), chunks.data(), chunks.size() * sizeof(OptChunk), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(q->d_first.get(), first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice));
    q->h_slots.assign(reinterpret_cast<const OptSlot*>(slots), reinterpret_cast<const OptSlot*>(slots) + n);
    *out = q.release();
    return 0;
}

// New pointers for the same tensors (same count, same element counts): e.g. the gradients of a step landed in a fresh buffer.
// One asynchronous upload on `stream`; no allocation, no synchronisation.
int rdmi_opt_update_slots(rdmi_opt* q, const rdmi_opt_slot* slots, int n, void* stream) {
    if (!q || !slots) return fail("rdmi_opt_update_slots: null argument");
    if (n != q->nslots) return fail("rdmi_opt_update_slots: %d slots, the table was created with %d", n, q->nslots);
    const OptSlot* ns = reinterpret_cast<const OptSlot*>(slots);
    for (int t = 0; t < n; ++t) {
        if (ns[t].n != q->h_slots[(size_t)t].n) return fail("rdmi_opt_update_slots: slot %d changed its element count", t);
        if (!slots[t].param || !slots[t].grad || !slots[t].exp_avg || !slots[t].exp_avg_sq) return fail("rdmi_opt_update_slots: slot %d has a null pointer", t);
        if ((q->h_slots[(size_t)t].ema == nullptr) != (ns[t].ema == nullptr)) return fail("rdmi_opt_update_slots: slot %d gained or lost its EMA shadow", t);
    }
    q->h_slots.assign(ns, ns + n);
    HIP_OK(hipMemcpyAsync(q->d_slots.get(), q->h_slots.data(), (size_t)n * sizeof(OptSlot), hipMemcpyHostToDevice, (hipStream_t)stream));
    return 0;
}

int rdmi_opt_destroy(rdmi_opt* q) {
    delete q;
    return 0;
}

int rdmi_opt_step(rdmi_opt* q, const rdmi_opt_hyper* hy, float* total_norm_out, void* stream) {
    if (!q || !hy) return fail("rdmi_opt_step: null argument");
    if (hy->step < 1) return fail("rdmi_opt_step: step=%d (the first update is step 1)", hy->step);
    hipStream_t s = (hipStream_t)stream;
    OptHyper h{};
    h.lr = hy->lr; h.beta1 = hy->beta1; h.beta2 = hy->beta2; h.eps = hy->eps; h.weight_decay = hy->weight_decay; h.decoupled_wd = hy->decoupled_wd;
    // python-float arithmetic of torch.optim.adam._single_tensor_adam, rounded to fp32 where the kernel consumes it
    const double bc1 = 1.0 - std::pow((double)hy->beta1_d, (double)hy->step), bc2 = 1.0 - std::pow((double)hy->beta2_d, (double)hy->step);
    h.step_size = (float)((double)hy->lr_d / bc1);
    h.bc2_sqrt = (float)std::sqrt(bc2);
    h.one_minus_beta1 = (float)(1.0 - hy->beta1_d); h.one_minus_beta2 = (float)(1.0 - hy->beta2_d);
    h.max_norm = hy->max_norm;
    h.one_minus_ema_decay = (float)(1.0 - hy->ema_decay_d);
    h.write_back_grad = hy->write_back_grad;
    hipLaunchKernelGGL(opt_sumsq_kernel, dim3((unsigned)q->nchunks), dim3(RDMI_THREADS), 16, s, (const OptSlot*)q->d_slots.get(), (const OptChunk*)q->d_chunks.get(), q->d_partial.get());
    hipLaunchKernelGGL(opt_norm_kernel, dim3(1), dim3(RDMI_THREADS), RDMI_THREADS * sizeof(float), s, (const float*)q->d_partial.get(), (const int*)q->d_first.get(), q->nslots,
                       hy->max_norm, q->d_norm.get());
    hipLaunchKernelGGL(opt_adam_ema_kernel, dim3((unsigned)q->nchunks), dim3(RDMI_THREADS), 0, s, (const OptSlot*)q->d_slots.get(), (const OptChunk*)q->d_chunks.get(), h,
                       (const float*)q->d_norm.get());
    HIP_OK(hipGetLastError());
    if (total_norm_out) HIP_OK(hipMemcpyAsync(total_norm_out, q->d_norm.get(), sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

int rdmi_get_tap(rdmi_ctx* c, const char* name, float* dst, size_t dst_numel, int* C, int* H, int* W, void* stream) {
    if (!c || !name || !dst) return fail("null argument");
    hipStream_t s = (hipStream_t)stream;
    const std::string nm(name);
    if (c->tiled) {      // the tiled plan never reuses a tensor: the output of a block is its last conv (Conv_1 / NIN_3)
        for (auto it = c->tiled->launches.rbegin(); it != c->tiled->launches.rend(); ++it) {
            const TConvL* cv = std::get_if<TConvL>(&it->op);
            if (!cv || !(it->name == nm || it->name == nm + ".Conv_1" || it->name == nm + ".NIN_3")) continue;
            const TConvArgs& a = cv->a;
            if (C) *C = a.Cout; if (H) *H = a.Ho; if (W) *W = a.Wo;
            const size_t per = (size_t)a.Cout * a.Ho * a.Wo;
            const int nb = (int)std::min<size_t>(dst_numel / per, (size_t)c->max_batch);
            hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((unsigned)ceil_div((int)(nb * per), RDMI_THREADS)), dim3(RDMI_THREADS), 0, s, (const float*)a.out, dst, nb,
                               a.Ho * a.Wo, a.Cout, 0);
            HIP_OK(hipGetLastError());
            return 0;
        }
        return fail("no activation named '%s' in the tiled plan", name);
    }
    if (!c->debug_taps) return fail("taps need RDMI_DEBUG_TAPS=1 at rdmi_create (buffers are reused otherwise)");
    if (nm == "temb") {
        if (C) *C = c->temb; if (H) *H = 1; if (W) *W = 1;
        HIP_OK(hipMemcpyAsync(dst, c->d_temb.get(), std::min(dst_numel, (size_t)c->max_batch * c->temb) * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    for (auto& t : c->tensors) {
        if (t.name != nm) continue;
        if (C) *C = t.C; if (H) *H = t.H; if (W) *W = t.W;
        const size_t per = t.per_sample();
        const int nb = (int)std::min<size_t>(dst_numel / per, (size_t)c->max_batch);
        hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((unsigned)ceil_div((int)(nb * per), RDMI_THREADS)), dim3(RDMI_THREADS), 0, s,
                           (const float*)(c->ws.get() + t.off * (size_t)c->max_batch), dst, nb, t.H * t.W, t.C, c->arch.compute_dtype == 1 ? 1 : 0);
        HIP_OK(hipGetLastError());
        return 0;
    }
    return fail("no activation named '%s'", name);
}

int rdmi_set_profiling(rdmi_ctx* c, int enabled) {
    if (!c) return fail("null context");
    c->profiling = enabled != 0;
    c->prof.clear();
    c->ev_used = 0;
    return 0;
}

int rdmi_get_profile(rdmi_ctx* c, int index, const char** kernel_name, double* total_ms, long* launches, double* flops) {
    if (!c || index < 0 || index >= (int)c->prof.size()) return 1;
    const ProfEntry& e = c->prof[(size_t)index];
    if (kernel_name) *kernel_name = e.name.c_str();
    if (total_ms) *total_ms = e.ms;
    if (launches) *launches = e.launches;
    if (flops) *flops = e.flops;
    return 0;
}

}  // extern "C"
