// The FUSED plan (kernel: csrc/unet_kernel.h): NCSNpp.forward as ONE workgroup-resident launch, a program of FOps over LDS tensors.
// Included by rdmi.hip after FwdIn, next to tiled_plan.h; everything that plans, binds and launches these programs lives here.
// FusedProg / FusedPlan: a program and the context's set of them (rdmi_ctx::fused).  FusedBuilder: LDS arena, row tables, op emission
// (FConv names the fields of one conv op).  fused_resblock / fused_attn emit a block and say what the training program stashes and whose
// Dropout_0 applies; FusedWalk holds the four steps (down block, up block, downsample, upsample) that build_fused_program_pass walks in
// its three sections.  bind_fused_params is the only switch over patch fields (repack and training step), run_fused the launch.
// Parameter names become indices while a program is built: an unknown name fails there, never at a repack.
#pragma once

namespace {

enum { F_GAMMA, F_BETA, F_BIAS, F_W };                  // the descriptor fields that hold parameter-dependent pointers
struct FPatch { int op, field, param; size_t arena_off; };     // param: index in rdmi_ctx::params, or -1: the weight arena at arena_off

struct FusedProg {
    int S = 1; bool ok = false; std::string why;     // why: the reason the program could not be built (the layer plan runs instead)
    std::vector<FOp> fprog;              // host copy; parameter pointers are patched at repack time
    std::vector<FPatch> fpatch; std::vector<short> ftabs;
    std::vector<std::string> fdesc;      // one line per fused op
    dev_ptr<FOp> d_fprog; dev_ptr<short> d_ftabs; dev_ptr<float> d_spill; size_t spill_per_sample = 0;
    UnetArgs fargs{}; size_t fused_lds = 0;
    bool coop = false; int n_xchg = 0; dev_ptr<unsigned long long> d_xbuf; dev_ptr<int> d_coop_err; int max_nb = 0;     // co-operative program
    bool train = false;                  // the training forward's program (stashes every layer output, applies Dropout_0): never picked for inference
};

struct FusedPlan {                       // one program per samples-per-workgroup value
    std::vector<FusedProg> progs;
    std::map<std::string, int> dense_off;          // Dense_0 column offset of every res block (build_plan)
    dev_ptr<long long> d_stamps;                   // diagnostic (RDMI_STAMPS=1), shared by the programs that record stamps
    int s_min_wg = 256;                            // a program with S samples per workgroup is used from batch s_min_wg * S (RDMI_S_MIN_WG: tests)
    bool use_coop = true;                          // RDMI_COOP=0: never select the co-operative program (A/B, tests)
    int coop_stride = 1;                           // ids of a group's members are this far apart (RDMI_COOP_STRIDE).  1: under round-robin placement member m of every
                                                   // group sits on XCDs m and m + 4, so an XCD's L2 only ever holds ITS quarter of the shared weights (2.5 MB: it stays
                                                   // resident from one launch to the next); 8 would put a whole group on one XCD (cheaper exchanges, 4x the weights per L2).
                                                   // Measured at B = 128: 821 vs 837 us per update.  Speed only: the exchange is correct under any placement.
    unsigned coop_epoch = 0;                       // tag base of the next co-operative launch
    int last_prog = 0;                             // index in progs of the program the last forward ran (diagnostics)
    int train_prog = -1;                           // index in progs of the training forward's program (-1: the layer plan runs the training forward)
    const FusedProg* pick(int NB) const {
        // a batch that leaves CUs to spare at one sample per workgroup and fits the chip in ONE wave of workgroups: the co-operative
        // program (groups of four CUs share the low-resolution weights); larger batches: the program with the most samples per
        // workgroup that still fills the chip
        if (use_coop) for (auto& q : progs) if (q.ok && q.coop && !q.train && NB <= q.max_nb) return &q;
        const FusedProg* best = nullptr;
        for (auto& q : progs) if (q.ok && !q.coop && !q.train && (q.S == 1 || NB >= s_min_wg * q.S) && (!best || q.S > best->S)) best = &q;
        return best;
    }
    bool ready() const { return !progs.empty() && progs[0].ok; }
    const FusedProg* training() const { return train_prog >= 0 && progs[(size_t)train_prog].ok ? &progs[(size_t)train_prog] : nullptr; }
};
inline bool fused_ready(const rdmi_ctx* c) { return c->fused && c->fused->ready(); }

struct FusedBuilder {
    rdmi_ctx* c;
    FusedProg& prog;                           // the program being built
    static constexpr int LDS_TOTAL = 160 * 1024;
    struct Blk { int off, size; };
    std::vector<Blk> freel;
    int arena_lo = 0, high_water = 0;
    std::map<std::string, int> tabcache;       // geometry key -> encoded table reference (region << 24 | offset in shorts)
    std::vector<short> tabs1;                  // region 1: tables of the multi-sample (low-resolution) section, resident in LDS only during it
    int tab1_lds = 0;                          // LDS byte offset of region 1 (an arena block of the low-resolution section)
    struct LT { int off = -1, C = 0, H = 0, W = 0, rs = 0, bytes = 0, ns = 1; bool pm = false; int hw() const { return H * W; } int rows() const { return ns * H * W; } };
    // pm: the rows are PHASE-MAJOR (output of the folded upsample conv, conv_up4): pixel (2y + py, 2x + px) of the H x W grid sits in row
    // (2 py + px) * (H/2 * W/2) + y * W/2 + x.  Readers go through a row map (gather_cat) -- no op takes such a tensor as a plain grid.
    static int pm_row(int H, int W, int y, int x) { return (2 * (y & 1) + (x & 1)) * ((H / 2) * (W / 2)) + (y / 2) * (W / 2) + x / 2; }
    int S = 1;                      // samples per workgroup of the program being built
    bool coop = false;              // co-operative program: S = 4 samples per GROUP of four workgroups (unet_kernel.h: fop_conv_coop)
    bool train = false;             // training forward: stash every layer-plan tensor, Dropout_0 in the fused GroupNorm_1 epilogues
    std::map<std::string, int> lp_tensor, lp_op;      // layer-plan tensor / op indices by name (train)
    int n_xchg = 0;                 // exchanges emitted so far
    int xslot_granules = 0;         // largest exchanged block, in 8-byte granules
    struct PendX { bool on = false; LT t; } pendx;      // output of the last co-operative 3x3 conv: exchanged before the next op is emitted
    int cur_samp = 0;               // sample slot the emitted ops belong to; -1: ops cover all S samples (low-resolution section)
    int multi_slot_off = -1;        // LDS offset of the per-(sample, group) partial-sum slots of multi-sample fused GroupNorms
    int ns_now() const { return cur_samp < 0 ? S : 1; }
    int shift_of(int hw) { int sh = 0; while ((1 << sh) < hw) ++sh; if (cur_samp < 0 && (1 << sh) != hw) fail_("multi-sample ops need a power-of-two pixel count"); return cur_samp < 0 ? sh : 0; }
    size_t spill_floats = 0;
    bool failed = false;
    std::string why;
    int gn_slot_off = 0;            // LDS byte offset of the fused-GroupNorm partial-sum slots (2 KiB)
    bool gn_fuse = true;            // RDMI_NO_GNFUSE=1 keeps every GroupNorm its own op (A/B and debugging)

    void fail_(const std::string& m) { if (!failed) { failed = true; why = m; } }

    // ---- names, resolved while the program is built
    int param(const std::string& name) const { return c->pindex.at(name); }        // parameter index
    size_t w(const std::string& key) const { return c->wmap.at(key); }              // packed-weight arena offset

    // ---- LDS arena: first-fit with coalescing free list
    void arena_init(int lo) { arena_lo = lo; freel.clear(); freel.push_back({lo, LDS_TOTAL - lo}); high_water = lo; }
    int alloc_bytes(int n) {
        n = (n + 15) & ~15;
        for (size_t i = 0; i < freel.size(); ++i)
            if (freel[i].size >= n) {
                const int o = freel[i].off;
                freel[i].off += n; freel[i].size -= n;
                if (freel[i].size == 0) freel.erase(freel.begin() + (long)i);
                high_water = std::max(high_water, o + n);
                return o;
            }
        {
            std::string fl;
            for (auto& f : freel) fl += " [" + std::to_string(f.off) + "+" + std::to_string(f.size) + "]";
            fail_("LDS arena exhausted at op " + std::to_string(prog.fprog.size()) + " (need " + std::to_string(n) + " B; free:" + fl + ")");
        }
        return arena_lo;
    }
    int alloc_top(int n) {                      // odd-sized scratch (Vt, P): carve from the END of the highest block that fits
        n = (n + 15) & ~15;
        for (size_t k = freel.size(); k-- > 0;)
            if (freel[k].size >= n) {
                const int o = freel[k].off + freel[k].size - n;
                freel[k].size -= n;
                if (freel[k].size == 0) freel.erase(freel.begin() + (long)k);
                high_water = std::max(high_water, o + n);
                return o;
            }
        return alloc_bytes(n);
    }
    void free_bytes(int off, int n) {
        n = (n + 15) & ~15;
        freel.push_back({off, n});
        std::sort(freel.begin(), freel.end(), [](const Blk& a, const Blk& b) { return a.off < b.off; });
        for (size_t i = 0; i + 1 < freel.size();)
            if (freel[i].off + freel[i].size == freel[i + 1].off) { freel[i].size += freel[i + 1].size; freel.erase(freel.begin() + (long)i + 1); }
            else ++i;
    }
    LT talloc(int C, int H, int W) {
        LT t; t.C = C; t.H = H; t.W = W; t.ns = ns_now(); t.rs = C + 4; t.bytes = t.ns * H * W * t.rs * 4; t.off = alloc_bytes(t.bytes);
        return t;
    }
    void tfree(LT& t) { if (t.off >= 0) free_bytes(t.off, t.bytes); t.off = -1; }

    // ---- row tables (int16), deduplicated by geometry
    int add_table(const std::string& key, const std::vector<short>& v) {
        auto it = tabcache.find(key);
        if (it != tabcache.end()) return it->second;
        const int region = (S > 1 && cur_samp < 0) ? 1 : 0;
        std::vector<short>& tb = region ? tabs1 : prog.ftabs;
        while (tb.size() % 2) tb.push_back(-1);
        const int off = (int)tb.size() | (region << 24);
        tb.insert(tb.end(), v.begin(), v.end());
        tabcache[key] = off;
        return off;
    }
    // tap table of a conv reading tensor (Hs x Ws) seen as a virtual (Hv x Wv) grid (nearest), output (Ho x Wo)
    int tap_table(int Hs, int Ws, int Hv, int Wv, int Ho, int Wo, int stride, int pad_lo, int tap) {
        char key[128];
        const int ns = ns_now();                       // multi-sample: block-diagonal (row s*HWo + p reads source row s*HWs + ...)
        snprintf(key, sizeof key, "tap:%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", Hs, Ws, Hv, Wv, Ho, Wo, stride, pad_lo, tap, ns);
        const int Mpad = pad16(ns * Ho * Wo);
        std::vector<short> v((size_t)Mpad, (short)-1);
        for (int m = 0; m < ns * Ho * Wo; ++m) {
            const int sm = m / (Ho * Wo), pm = m % (Ho * Wo);
            const int oy = pm / Wo, ox = pm % Wo;
            const int iy = oy * stride + tap / 3 - pad_lo, ix = ox * stride + tap % 3 - pad_lo;
            if (iy < 0 || iy >= Hv || ix < 0 || ix >= Wv) continue;
            const int sy = std::min((int)std::floor(iy * ((float)Hs / Hv)), Hs - 1);
            const int sx = std::min((int)std::floor(ix * ((float)Ws / Wv)), Ws - 1);
            v[(size_t)m] = (short)(sm * Hs * Ws + sy * Ws + sx);
        }
        return add_table(key, v);
    }
    int ident_table(int M) {
        const int Mpad = pad16(M);
        std::vector<short> v((size_t)Mpad, (short)-1);
        for (int m = 0; m < M; ++m) v[(size_t)m] = (short)m;
        return add_table("id:" + std::to_string(M), v);
    }
    int map_table(int Hs, int Ws, int Hd, int Wd, bool pm = false) {      // nearest map as a GATHER row map (pm: onto a phase-major source, LT::pm)
        std::vector<short> v((size_t)Hd * Wd);
        for (int y = 0; y < Hd; ++y)
            for (int x = 0; x < Wd; ++x) {
                const int sy = std::min((int)std::floor(y * ((float)Hs / Hd)), Hs - 1);
                const int sx = std::min((int)std::floor(x * ((float)Ws / Wd)), Ws - 1);
                v[(size_t)y * Wd + x] = (short)(pm ? pm_row(Hs, Ws, sy, sx) : sy * Ws + sx);
            }
        char key[64];
        snprintf(key, sizeof key, "map:%d,%d,%d,%d,%d", Hs, Ws, Hd, Wd, pm ? 1 : 0);
        return add_table(key, v);
    }
    // Tap table t = 2 ty + tx of the folded upsample conv over a source of Hs x Ws = 16 pixels: entry [16 p + i] is the source row that tap
    // (ty, tx) of phase p = 2 py + px reads for source pixel i = y * Ws + x, i.e. pixel (y + ty - 1 + py, x + tx - 1 + px), or -1 (zero row).
    // An upsampled pixel lies outside the 2Hs x 2Ws grid exactly when its source pixel lies outside Hs x Ws: the padding carries over.
    int up4_table(int Hs, int Ws, int tap) {
        std::vector<short> v((size_t)4 * Hs * Ws, (short)-1);
        for (int p = 0; p < 4; ++p)
            for (int y = 0; y < Hs; ++y)
                for (int x = 0; x < Ws; ++x) {
                    const int sy = y + (tap >> 1) - 1 + (p >> 1), sx = x + (tap & 1) - 1 + (p & 1);
                    if (sy >= 0 && sy < Hs && sx >= 0 && sx < Ws) v[(size_t)p * Hs * Ws + y * Ws + x] = (short)(sy * Ws + sx);
                }
        char key[64];
        snprintf(key, sizeof key, "up4:%d,%d,%d", Hs, Ws, tap);
        return add_table(key, v);
    }

    // ---- op emission.  Table offsets are emitted in SHORTS relative to the table region and turned into LDS
    //      byte offsets once the region's base is known (build_fused_program_pass).
    FOp blank(int kind) {
        FOp o;
        std::memset(&o, 0, sizeof o);
        o.kind = kind; o.a_off = -1; o.b_off = -1; o.a_map_off = -1; o.dense_off = -1; o.resid_off = -1; o.scale = 1.f; o.src_off = -1; o.gn_off = -1; o.samp = cur_samp; o.drop_op = -1;
        return o;
    }
    int emit(const FOp& o) { flush_xchg(); prog.fprog.push_back(o); return (int)prog.fprog.size() - 1; }
    // all-gather of tensor t (column slices of 32 per member) between the four members; t2: a second tensor of the same shape
    int emit_xchg(const LT& t, const LT* own_rows_src) {
        FOp o = blank(FOP_XCHG);
        o.dst_off = t.off; o.dst_rs = t.rs; o.xidx = n_xchg++;
        if (own_rows_src) {          // row slices: every member contributes its sample's rows (all columns)
            o.a_hw = 1; o.rows = own_rows_src->hw(); o.C = t.C; o.a_off = own_rows_src->off; o.a_rs = own_rows_src->rs;
            if (own_rows_src->C != t.C || t.rows() != 4 * o.rows) fail_("exchange: row-slice shapes");
        } else {
            o.a_hw = 0; o.rows = t.rows(); o.C = t.C / 4;
        }
        if (o.C < 32 || o.C > 128 || (o.C & (o.C - 1)) || o.rows * o.C > 512) fail_("exchange: block of " + std::to_string(o.rows) + " x " + std::to_string(o.C));
        xslot_granules = std::max(xslot_granules, 2 * o.rows * o.C);      // room for a second tensor (<= 1024 granules = 512 pairs: one per thread)
        prog.fprog.push_back(o);
        return (int)prog.fprog.size() - 1;
    }
    void flush_xchg() { if (pendx.on) { pendx.on = false; emit_xchg(pendx.t, nullptr); } }
    void patch(int op, int field, int param, size_t arena_off = 0) { prog.fpatch.push_back({op, field, param, arena_off}); }      // param < 0: the arena at arena_off

    FOp gather_into(const LT& dst) {
        FOp o = blank(FOP_GATHER);
        o.dst_off = dst.off; o.dst_rs = dst.rs; o.rows = dst.rows(); o.C = dst.C;
        return o;
    }
    void gather_x(const LT& dst) {               // network input -> LDS [HW][16+4]
        FOp o = gather_into(dst);
        o.CA = c->arch.channels; o.CB = 0; o.a_off = -2; o.a_hw = dst.hw(); o.hw_shift = shift_of(dst.hw());
        emit(o);
    }
    // dst = a tensor parked in this workgroup's spill slot `spill` ([n][hw][C]); single- or multi-sample by the current mode
    void gather_g(const LT& dst, size_t spill) {
        FOp o = gather_into(dst);
        o.CA = dst.C; o.CB = 0; o.a_off = -1; o.a_hw = dst.hw(); o.a_mod = 0; o.hw_shift = shift_of(dst.hw());
        const int idx = emit(o);
        spill_fix.push_back({idx, spill, 2});
    }
    // dst = concat(A (LDS tensor, nearest-mapped onto dst's grid), B (global spill slot))
    void gather_cat(const LT& dst, const LT& A, size_t spillB, int CB) {
        FOp o = gather_into(dst);
        o.CA = A.C; o.CB = CB; o.a_off = A.off; o.a_rs = A.rs; o.a_hw = A.hw(); o.hw_shift = shift_of(dst.hw());
        if (A.H != dst.H || A.W != dst.W || A.pm) o.a_map_off = map_table(A.H, A.W, dst.H, dst.W, A.pm);
        if (A.pm && A.ns != 1) fail_("phase-major tensors are single-sample");
        const int idx = emit(o);
        spill_fix.push_back({idx, spillB, 1});
    }
    void copy_t(const LT& dst, const LT& src) {
        if (src.pm) fail_("copy of a phase-major tensor");
        FOp o = gather_into(dst);
        o.CA = src.C; o.CB = 0; o.a_off = src.off; o.a_rs = src.rs; o.a_hw = src.hw(); o.hw_shift = shift_of(dst.hw());
        emit(o);
    }
    struct SpillFix { int op; size_t off; int which; };      // which: 0 STORE destination, 1 GATHER source B, 2 GATHER source A
    // Per-sample sections of a multi-sample program are emitted once per sample slot: the spill slots they use must be the
    // SAME for every slot (the buffer is [slot][n][rows][C]); the first emission records them, the others replay them.
    std::vector<size_t> slot_log; size_t slot_pos = 0; bool slot_replay = false;
    std::vector<SpillFix> spill_fix;
    size_t spill_store(const LT& t) {            // LDS tensor -> this workgroup's slot of the spill buffer
        if (t.pm) fail_("spill of a phase-major tensor");
        FOp o = blank(FOP_STORE);
        o.dst_off = t.off; o.dst_rs = t.rs; o.rows = t.rows(); o.C = t.C; o.hw_shift = shift_of(t.hw());
        const int idx = emit(o);
        size_t off;
        if (slot_replay) { if (slot_pos >= slot_log.size()) { fail_("spill replay out of slots"); return 0; } off = slot_log[slot_pos++]; }
        else { off = spill_floats; spill_floats += (size_t)t.hw() * t.C; slot_log.push_back(off); }
        spill_fix.push_back({idx, off, 0});
        return off;
    }
    // GroupNorm (+SiLU) of tensor t (in place), or of `src` into t (copy form); `pre` is its parameter prefix.  When the tensor being
    // normalised is the output of the CONV op emitted just before (only STOREs in between), has 4-channel groups and the conv's tiling
    // gives every wave a single pass, the GroupNorm is folded into that conv's epilogue (FOp::gn_*) and no op is emitted.
    // drop_block (training program): this activation is Conv_1's input in res block drop_block, the layer-plan op of that exact name, whose Dropout_0 acts on it.
    static int conv_wave_rows(int ntiles) {          // WM of fop_conv: the 8 waves as WN along the column tiles x WM along the row tiles
        const int lWN = (ntiles >= 8 && (ntiles & 7) == 0) ? 3 : (ntiles >= 4 ? 2 : (ntiles >= 2 ? 1 : 0));
        return UW_WAVES >> lWN;
    }
    // Every single-sample fused GroupNorm of the finished program: the reader's slot count covers exactly the wave rows that park sums.
    void check_gn_slots() {
        for (size_t i = 0; i < prog.fprog.size(); ++i) {
            const FOp& o = prog.fprog[i];
            if (o.kind != FOP_CONV || o.gn_off < 0 || o.samp < 0) continue;
            const int WM = conv_wave_rows(o.Cout_pad >> 4);
            if (o.mtiles < 1 || o.mtiles > 4 * WM || o.gn_nslots != std::min(WM, o.mtiles) * 4 || (o.Cout / 4) * o.gn_nslots * 8 > 1024)
                fail_("fused GroupNorm of op " + std::to_string(i) + ": " + std::to_string(o.gn_nslots) + " partial-sum slots for " + std::to_string(o.mtiles) + " row tiles over " + std::to_string(WM) + " wave rows");
        }
    }
    bool try_fuse_gn(const LT& t, const std::string& pre, bool act, const LT* src, const std::string& drop_block) {
        if (!gn_fuse) return false;
        const LT& in = src ? *src : t;
        int j = (int)prog.fprog.size() - 1, jx = -1;
        while (j >= 0 && (prog.fprog[(size_t)j].kind == FOP_STORE || prog.fprog[(size_t)j].kind == FOP_XCHG)) { if (prog.fprog[(size_t)j].kind == FOP_XCHG) jx = j; --j; }
        if (j < 0) return false;
        FOp& p = prog.fprog[(size_t)j];
        if (p.coop && !pendx.on && (jx < 0 || prog.fprog[(size_t)jx].dst_off != in.off || prog.fprog[(size_t)jx].src_off >= 0)) return false;
        if (p.kind != FOP_CONV || p.dst_kind != 0 || p.gn_off >= 0 || p.dst_off != in.off || p.dst_rs != in.rs) return false;
        if (p.Cout != t.C || p.rows != t.rows() || t.C % 4 != 0 || std::min(t.C / 4, 32) * 4 != t.C) return false;      // Cg == 4 only
        const int ntiles = p.Cout_pad >> 4;
        const int WM = conv_wave_rows(ntiles), WN = UW_WAVES / WM;
        if (ntiles > WN || p.mtiles > 4 * WM) return false;                    // a wave would make several passes
        // Single-sample form: wave row wm parks its partial sums in slots wm * 4 + kq (fconv_epi) and the reader adds slots 0 .. nslots - 1
        // (fconv_gn_apply, two per float4).  Only wave rows that own a row tile enter fop_conv's tile loop, so the reader must stop at
        // min(WM, mtiles) * 4: the slots of the other wave rows hold whatever the op before left in LDS.  (The room check keeps the full
        // WM * 4, so which GroupNorms fold does not depend on the conv's height.)
        const int nslots = p.samp >= 0 ? std::min(WM, p.mtiles) * 4 : 4;
        if (p.samp >= 0) { if ((t.C / 4) * WM * 4 * 8 > 1024) return false; }
        else if (multi_slot_off < 0 || t.ns * (t.C / 4) * 32 > 4096 || (t.hw() != 16 && t.hw() != 4)) return false;        p.gn_off = t.off; p.gn_rs = t.rs; p.gn_act = act ? 1 : 0; p.gn_raw = src ? 1 : 0;
        p.gn_slot_off = p.samp >= 0 ? gn_slot_off : multi_slot_off; p.gn_nslots = nslots;
        p.eps = 1e-6f; p.inv_cnt = 1.0f / (float)(4 * t.hw());
        patch(j, F_GAMMA, param(pre + ".weight")); patch(j, F_BETA, param(pre + ".bias"));
        if (train && !drop_block.empty()) {
            auto it = lp_op.find(drop_block);
            if (it == lp_op.end()) fail_("training forward: no layer-plan op for " + pre);
            else if (c->ops[(size_t)it->second].dropout) p.drop_op = it->second;
        }
        if (p.coop) {        // the conv now also produces the activated tensor (own columns): it has to travel too
            if (pendx.on) {
                if (src) { pendx.on = false; const int ix = emit_xchg(in, nullptr); prog.fprog[(size_t)ix].src_off = t.off; prog.fprog[(size_t)ix].src_rs = t.rs; }
                // in-place form: the pending exchange of the conv's destination already carries the activated values
            } else if (src) { prog.fprog[(size_t)jx].src_off = t.off; prog.fprog[(size_t)jx].src_rs = t.rs; }
        }
        return true;
    }
    void gn(const LT& t, const std::string& pre, bool act, const LT* src = nullptr, const std::string& drop_block = "") {
        if (t.pm || (src && src->pm)) fail_("GroupNorm of a phase-major tensor");
        if (try_fuse_gn(t, pre, act, src, drop_block)) return;
        if (train && !drop_block.empty()) fail_("training forward: " + pre + " is not folded into its conv (Dropout_0 lives in that epilogue)");
        FOp o = blank(FOP_GN);
        if (src) { o.src_off = src->off; o.src_rs = src->rs; }
        o.dst_off = t.off; o.dst_rs = t.rs; o.rows = t.rows(); o.C = t.C;
        o.G = std::min(t.C / 4, 32); o.act = act ? 1 : 0; o.eps = 1e-6f; o.hw_shift = shift_of(t.hw());
        {
            // multi-sample ops spread the ns * G (sample, group) pairs over the workgroup: T lanes per pair
            const int pairs = t.ns * o.G, T = UW_THREADS / pairs, c4n = t.C / 4;
            o.logT = T == 32 ? 5 : (T == 16 ? 4 : (T == 64 ? 6 : (T == 8 ? 3 : 2)));
            o.logG = 0; while ((1 << o.logG) < o.G) ++o.logG;
            o.Cg = t.C / o.G;
            o.magic_c4n = (65536 + c4n - 1) / c4n; o.magic_Cg = (65536 + o.Cg - 1) / o.Cg;
            o.inv_cnt = 1.0f / (float)(o.Cg * t.hw());
            if ((1 << o.logT) != T || T * pairs != UW_THREADS) fail_("GroupNorm lanes-per-group not a power of two");
            if ((1 << o.logG) != o.G) fail_("GroupNorm group count not a power of two");
            if (t.ns * o.G * 8 > 1024) fail_("GroupNorm statistics of all samples exceed the scratch region");
            if (ceil_div(t.hw(), T) > 6 || o.Cg > 8) fail_("GroupNorm group too large for the register-resident statistics");
        }
        if (t.C % o.G != 0 || UW_THREADS % o.G != 0 || UW_THREADS / o.G > 64) fail_("GroupNorm shape C=" + std::to_string(t.C));
        const int idx = emit(o);
        patch(idx, F_GAMMA, param(pre + ".weight")); patch(idx, F_BETA, param(pre + ".bias"));
    }
    // One CONV op over LDS tensor `in`.  The defaults describe the common case: 3x3, stride 1, pad 1, on the source's own grid, into an LDS tensor.
    struct FConv {
        const LT* in = nullptr;                // source tensor
        int Hv = 0, Wv = 0, Ho = 0, Wo = 0;    // virtual grid the source is seen on (nearest) and output grid; 0: the source's own
        int stride = 1, pad = 1;
        int ntap = 9;                          // 9: 3x3; 1: 1x1 (stride and pad unused)
        size_t w = 0;                          // packed weight: arena offset
        int bias = -1; size_t bias_arena = 0;  // bias: parameter index, or (-1) a packed row of the arena at bias_arena
        int Cout = 0;
        int dst_kind = 0; const LT* dst = nullptr;      // FOp::dst_kind (0: LDS tensor dst; 2: the network output; 3: q | k | v split, first part to dst)
        float scale = 1.f;
        int dense_off = -1;                    // >= 0: add this block's Dense_0 column slice
        const LT* resid = nullptr;             // add this LDS tensor
        std::string stash;                     // training program: exact name of the layer-plan tensor that keeps a copy of the output ("": none)
    };
    // a spec with the weight packed under `pre`, the bias parameter pre + bias_suffix, and Cout output channels
    FConv conv_of(const std::string& pre, const char* bias_suffix, int Cout) const { FConv s; s.w = w(pre); s.bias = param(pre + bias_suffix); s.Cout = Cout; return s; }
    int conv(const FConv& s) {
        const LT& in = *s.in;
        const int Hv = s.Hv ? s.Hv : in.H, Wv = s.Wv ? s.Wv : in.W, Ho = s.Ho ? s.Ho : in.H, Wo = s.Wo ? s.Wo : in.W;
        FOp o = blank(FOP_CONV);
        const int ns = ns_now();
        if (in.pm || (s.resid && s.resid->pm) || (s.dst && s.dst->pm)) fail_("conv over a phase-major tensor");
        o.rows = ns * Ho * Wo; o.mtiles = pad16(o.rows) / 16; o.Cout = s.Cout; o.Cout_pad = pad16(s.Cout);
        o.ntap = s.ntap; o.hw_shift = shift_of(Ho * Wo);
        if (ns > 1 && s.dst_kind != 0) fail_("multi-sample convs write LDS tensors only");
        o.main_ph.lds_off = in.off; o.main_ph.rs = in.rs; o.main_ph.nch = pad16(in.C) / 16;
        if (in.C % 16 != 0) fail_("conv input channels not padded");
        for (int t = 0; t < s.ntap; ++t)
            o.tab_off[t] = s.ntap == 1 ? ident_table(ns * Ho * Wo) : tap_table(in.H, in.W, Hv, Wv, Ho, Wo, s.stride, s.pad, t);
        o.dense_off = s.dense_off; o.scale = s.scale; o.dst_kind = s.dst_kind;
        if (s.dst) { o.dst_off = s.dst->off; o.dst_rs = s.dst->rs; }
        if (s.resid) { o.resid_off = s.resid->off; o.resid_rs = s.resid->rs; }
        if (o.mtiles > 6) fail_("conv with more than 96 output rows per workgroup");
        const int idx = emit(o);
        patch(idx, F_W, -1, s.w);
        patch(idx, F_BIAS, s.bias, s.bias_arena);
        if (train && !s.stash.empty() && s.dst_kind == 0) {      // the layer plan keeps this conv's output in that tensor: the backward reads it there
            auto it = lp_tensor.find(s.stash);
            if (it == lp_tensor.end()) fail_("training forward: no layer-plan tensor '" + s.stash + "'");
            else {
                const Tensor& t = c->tensors[(size_t)it->second];
                FOp& q = prog.fprog[(size_t)idx];
                if (t.C != s.Cout || t.H * t.W != q.rows) fail_("training forward: tensor '" + s.stash + "' has another shape");
                q.stash = c->ws.get() + t.off * (size_t)c->max_batch;
                q.stash_bf16 = c->arch.compute_dtype == 1 ? 1 : 0;
            }
        }
        if (coop && cur_samp < 0) {      // low-resolution section of the co-operative program: column-sliced, K split over the waves
            FOp& q = prog.fprog[(size_t)idx];
            q.coop = 1;
            if (q.Cout_pad != 128 || q.mtiles != 1 || q.main_ph.nch % 4 != 0 || s.dst_kind != 0 || !s.dst || s.dst->C != 128)
                fail_("co-operative conv shape (Cout " + std::to_string(s.Cout) + ", " + std::to_string(q.mtiles) + " row tiles, " + std::to_string(q.main_ph.nch) + " chunks)");
            if (s.ntap == 9) { pendx.on = true; pendx.t = *s.dst; }      // the next conv contracts over this tensor: all-gather it
        }
        return idx;
    }
    // Can the 3x3 conv over the nearest-x2 upsampled `in` run folded (conv_up4)?  Inference programs only: the training backward needs the
    // unfolded weight gradient.  RDMI_NO_UP_FOLD=1 keeps the nine-tap op (A/B and debugging).
    bool up_fold_ok(const LT& in, int Hv, int Wv, int Cout) const {
        return !train && cur_samp >= 0 && !in.pm && Hv == 2 * in.H && Wv == 2 * in.W && up_fold_shape_ok(in.H, in.W, in.C, Cout) &&
               c->wmap.count("upsample." + std::to_string(c->arch.n_levels - 2) + ".Conv_0.up4") != 0;
    }
    // The same conv as FOUR 2x2 convs on the source grid, one per output phase (py, px): output pixel (2y + py, 2x + px) reads source rows
    // y - 1, y, y through the nearest map when py = 0 and y, y, y + 1 when py = 1 (columns alike), so the taps that share a source pixel
    // have their weights summed once at repack time (pack kind 5) -- 4 taps instead of 9.  Each phase is one 16-row tile with its own four
    // weight blocks (FOp::w_tile_stride); dst is written phase-major (LT::pm).  `pre`: the conv's parameter prefix.
    int conv_up4(const LT& in, const std::string& pre, int Cout, LT* dst) {
        FOp o = blank(FOP_CONV);
        o.rows = 4 * in.hw(); o.mtiles = 4; o.Cout = Cout; o.Cout_pad = pad16(Cout);
        o.ntap = 4; o.hw_shift = shift_of(o.rows);
        o.main_ph.lds_off = in.off; o.main_ph.rs = in.rs; o.main_ph.nch = in.C / 16;
        for (int t = 0; t < 4; ++t) o.tab_off[t] = up4_table(in.H, in.W, t);
        o.w_tile_stride = 4 * in.C * o.Cout_pad * (int)sizeof(float);
        o.dst_off = dst->off; o.dst_rs = dst->rs;
        // fop_conv honours w_tile_stride only where a single-tile pass takes fconv_main_t<.., 1, false, 8>: chunks per tap in whole eights, more
        // than 4 rows, a plain LDS destination; the packed block is square (kind 5 packs ch x ch)
        if (o.main_ph.nch % 8 != 0 || o.rows <= 4 || o.dst_kind != 0 || in.C != Cout || in.hw() != 16 || in.pm || cur_samp < 0 || dst->C != Cout || dst->hw() != o.rows)
            fail_("folded upsample conv: unsupported shape (" + std::to_string(in.H) + "x" + std::to_string(in.W) + " source, " + std::to_string(in.C) + " -> " + std::to_string(Cout) + " channels)");
        dst->pm = true;
        const int idx = emit(o);
        patch(idx, F_W, -1, w(pre + ".up4"));
        patch(idx, F_BIAS, param(pre + ".bias"));
        return idx;
    }
};

// ResnetBlockDDPMpp on LDS tensors.  xin: raw block input (consumed).  Returns the block output.
// When the block has a NIN shortcut (cin != cout, i.e. every concat-fed up block) the shortcut is evaluated FIRST
// into the output buffer, so GroupNorm_0 can then run in place on xin: no second copy of the (large) concat
// tensor is ever resident.  Identity-shortcut blocks keep xin raw for the residual and normalise a copy.
// Training program: Conv_0's output is kept as "<block>.Conv_0", Conv_1's as "<block>", and GroupNorm_1 carries <block>'s Dropout_0.
FusedBuilder::LT fused_resblock(FusedBuilder& b, const std::string& name, FusedBuilder::LT& xin, int cout, int dense_off) {
    using LT = FusedBuilder::LT;
    using FConv = FusedBuilder::FConv;
    const bool nin = xin.C != cout;
    FConv c0 = b.conv_of(name + ".Conv_0", ".bias", cout), c1 = b.conv_of(name + ".Conv_1", ".bias", cout);
    c0.dense_off = dense_off; c0.stash = name + ".Conv_0";
    c1.scale = (float)(1.0 / std::sqrt(2.0)); c1.stash = name;
    LT out, xact;
    if (nin) {
        out = b.talloc(cout, xin.H, xin.W);
        FConv sc = b.conv_of(name + ".NIN_0", ".b", cout);
        sc.in = &xin; sc.ntap = 1; sc.dst = &out;
        b.conv(sc);
        b.gn(xin, name + ".GroupNorm_0", true);
    } else {
        xact = b.talloc(xin.C, xin.H, xin.W);
        b.gn(xact, name + ".GroupNorm_0", true, &xin);
    }
    LT& a0 = nin ? xin : xact;                   // Conv_0's activated input
    LT h1 = b.talloc(cout, xin.H, xin.W);
    c0.in = &a0; c0.dst = &h1;
    b.conv(c0);
    b.tfree(a0);
    b.gn(h1, name + ".GroupNorm_1", true, nullptr, name);
    if (!nin) out = b.talloc(cout, xin.H, xin.W);
    c1.in = &h1; c1.dst = &out; c1.resid = nin ? &out : &xin;
    b.conv(c1);
    b.tfree(h1);
    if (!nin) b.tfree(xin);
    return out;
}

// AttnBlockpp on an LDS tensor (consumed).  Returns the block output.  Training program: NIN_3's output is kept as "<name>".
FusedBuilder::LT fused_attn(FusedBuilder& b, const std::string& name, FusedBuilder::LT& x) {
    using LT = FusedBuilder::LT;
    rdmi_ctx* c = b.c;
    const int C = x.C, H = x.H, W = x.W, L = H * W, Lpad = pad16(L);
    if (C != 64 || Lpad > 96) { b.fail_("attention: only C=64, H*W<=96 is built"); return x; }
    if (b.cur_samp < 0) { b.fail_("attention inside the multi-sample (low-resolution) section is not built"); return x; }
    LT xn = b.talloc(C, H, W);
    b.gn(xn, name + ".GroupNorm_0", false, &x);
    // Inference programs fold NIN_3 into the value projection (weights packed as ".qkv3f" / ".bqkvf"): the attention op then writes
    // (P V' + b3 + x) / sqrt2 itself and the 1x1 NIN_3 conv -- 10-15 k cycles of almost pure per-op overhead, five times per forward --
    // disappears.  The training forward keeps the reference's op sequence (the backward needs the tensor between P V and NIN_3).
    const bool fold3 = !b.train && std::getenv("RDMI_NO_ATTN_FOLD") == nullptr;
    // ... and the k projection into q (k_fold_shape_ok; ".qv2f" / ".bqvf"): no k tensor, the attention op reads xn as K, so xn lives
    // until after that op, in place of the k tensor of the same size.  (fop_attn clamps key rows to L - 1: nothing is asked of xn's rows beyond L.)
    const bool foldk = fold3 && k_fold_shape_ok(C, L) && c->wmap.count(name + ".qv2f") != 0;
    const int NP = foldk ? 2 : 3;
    LT q = b.talloc(C, H, W), k = foldk ? xn : b.talloc(C, H, W);
    const int ps = Lpad + 4;
    const int vt_bytes = C * ps * 4, p_bytes = L * ps * 4;
    const int vt_off = b.alloc_top(vt_bytes);
    {   // q, k, v in one contraction over the dedicated packing [C/16][3C][16] (wmap key ".qkv3"; [C/16][2C][16] under the k fold)
        FusedBuilder::FConv s;
        s.in = &xn; s.ntap = 1; s.w = b.w(name + (foldk ? ".qv2f" : fold3 ? ".qkv3f" : ".qkv3")); s.bias_arena = b.w(name + (foldk ? ".bqvf" : fold3 ? ".bqkvf" : ".bqkv"));
        s.Cout = NP * C; s.dst_kind = 3; s.dst = &q;
        FOp& o = b.prog.fprog[(size_t)b.conv(s)];
        o.dst2_off = foldk ? q.off : k.off; o.dst3_off = vt_off; o.dst3_rs = ps; o.split_C = C;
        // the single-pass projection (fconv_qkv): the training kernel holds its three-projection form, the inference kernels the two-projection
        // form only -- an inference program without the k fold (RDMI_NO_K_FOLD=1, numerical A/B) runs the generic split conv
        o.qkv1 = (std::getenv("RDMI_NO_QKV1") == nullptr && (b.train || foldk) && o.ntap == 1 && o.main_ph.nch == 4 && o.Cout_pad == NP * 64 && C == 64 && o.mtiles <= 6) ? 1 : 0;
        if (foldk && !o.qkv1) b.fail_("attention: the k-folded projection needs the single-pass form");
    }
    if (!foldk) b.tfree(xn);
    const int p_off = b.alloc_top(p_bytes);
    // Under the k fold x, xn, q, Vt and P are all live here (xn used to be gone by now): the output goes where q is -- the op reads q
    // only in its score phase, which a barrier separates from the P V' phase that writes the output.
    LT o = foldk ? q : b.talloc(C, H, W);
    {
        FOp a = b.blank(FOP_ATTN);
        a.q_off = q.off; a.k_off = k.off; a.qk_rs = q.rs; a.k_rs = k.rs; a.vt_off = vt_off; a.p_off = p_off; a.ps = ps;
        a.L = L; a.Lpad = Lpad; a.C = C; a.att_scale = 1.0f / std::sqrt((float)C);
        a.dst_off = o.off; a.dst_rs = o.rs;
        if (fold3) { a.resid_off = x.off; a.resid_rs = x.rs; a.scale = (float)(1.0 / std::sqrt(2.0)); }
        const int ia = b.emit(a);
        if (fold3) b.patch(ia, F_BIAS, b.param(name + ".NIN_3.b"));
    }
    if (!foldk) b.tfree(q);
    b.tfree(k);                                  // under the k fold: xn
    b.free_bytes(vt_off, vt_bytes); b.free_bytes(p_off, p_bytes);
    if (fold3) { b.tfree(x); return o; }
    LT out = b.talloc(C, H, W);
    FusedBuilder::FConv s = b.conv_of(name + ".NIN_3", ".b", C);
    s.in = &o; s.ntap = 1; s.dst = &out;
    s.scale = (float)(1.0 / std::sqrt(2.0)); s.resid = &x; s.stash = name;
    b.conv(s);
    b.tfree(o);
    b.tfree(x);
    return out;
}

// The running state of a walk over the network (RD/models/ncsnpp.py:268-338) and its four steps.  build_fused_program_pass walks level 0
// once per sample slot, the low-resolution levels once, and level 0 on the way up once per slot again: all three through these.
struct FusedWalk {
    using LT = FusedBuilder::LT;
    FusedBuilder& b;
    const Layout& L;
    const std::map<std::string, int>& dense_off;
    struct HS { size_t spill; int C, H, W; };
    std::vector<HS> hs;                               // the skip stack
    LT h;                                             // the running tensor: ch channels on an H x W grid
    int ch = 0, H = 0, W = 0;

    // resblock, optional attention, spill (push: the spilled tensor becomes a skip; the replayed sample slots of level 0 do not push again)
    void down_block(int d, bool push) {
        const BlockSpec& bs = L.down[(size_t)d];
        h = fused_resblock(b, bs.name, h, bs.cout, dense_off.at(bs.name));
        ch = bs.cout;
        if (bs.attn) h = fused_attn(b, "down_attn." + std::to_string(d), h);
        const size_t sp = b.spill_store(h);
        if (push) hs.push_back({sp, ch, H, W});
    }
    // pop skip, gather concat (h is gathered, nearest, onto the skip's grid), resblock, optional attention
    void up_block(int u) {
        const BlockSpec& bs = L.up[(size_t)u];
        const HS sk = hs.back();
        hs.pop_back();
        LT cat = b.talloc(ch + sk.C, sk.H, sk.W);
        b.gather_cat(cat, h, sk.spill, sk.C);
        b.tfree(h);
        H = sk.H; W = sk.W;
        h = fused_resblock(b, bs.name, cat, bs.cout, dense_off.at(bs.name));
        ch = bs.cout;
        if (bs.attn) h = fused_attn(b, "up_attn." + std::to_string(u), h);
    }
    // the stride-2 conv below level i (training program: its output is kept as "downsample.<i>")
    void downsample(int i) {
        const std::string nm = "downsample." + std::to_string(i);
        FusedBuilder::FConv s = b.conv_of(nm + ".Conv_0", ".bias", ch);
        s.in = &h; s.Ho = (H + 1 - 3) / 2 + 1; s.Wo = (W + 1 - 3) / 2 + 1; s.stride = 2; s.pad = 0; s.stash = nm;
        LT o = b.talloc(ch, s.Ho, s.Wo);
        s.dst = &o;
        b.conv(s);
        b.tfree(h);
        h = o; H = s.Ho; W = s.Wo;
    }
    // nearest x2 + 3x3 conv number k (training program: kept as "upsample.<k>"); the one onto level 0 runs folded where conv_up4 takes it
    void upsample(int k) {
        const std::string nm = "upsample." + std::to_string(k);
        LT o = b.talloc(ch, 2 * H, 2 * W);
        if (k == b.c->arch.n_levels - 2 && b.up_fold_ok(h, 2 * H, 2 * W, ch)) b.conv_up4(h, nm + ".Conv_0", ch, &o);
        else {
            FusedBuilder::FConv s = b.conv_of(nm + ".Conv_0", ".bias", ch);
            s.in = &h; s.Hv = s.Ho = 2 * H; s.Wv = s.Wo = 2 * W; s.dst = &o; s.stash = nm;
            b.conv(s);
        }
        b.tfree(h);
        h = o; H *= 2; W *= 2;
    }
};

// How many workgroups of the fused kernel the device holds at once (one per CU: each takes the CU's whole LDS).
int resident_workgroups() {
#ifdef RDMI_EMU
    return 256;
#else
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return cus;
#endif
}

int build_fused_program_pass(rdmi_ctx* c, FusedProg& q, int S, int TAB_RESERVE, int TAB1_RESERVE, int* tab_used, int* tab1_used, bool coop, bool train) {
    using LT = FusedBuilder::LT;
    const rdmi_arch& a = c->arch;
    q.S = S; q.train = train;
    FusedBuilder b{c, q};
    b.S = S; b.coop = coop; b.train = train;
    if (train) {
        for (size_t i = 0; i < c->tensors.size(); ++i) b.lp_tensor[c->tensors[i].name] = (int)i;
        for (size_t i = 0; i < c->ops.size(); ++i) b.lp_op[c->ops[i].name] = (int)i;
    }
    const int nslot0 = coop ? 1 : S;                  // how often the full-resolution sections are emitted (co-operative: the member's own sample only)
    const Layout L = build_layout(c);
    FusedWalk w{b, L, c->fused->dense_off};
    // LDS: [row tables] [zero row] [GN stats] [tensor arena]
    const int zero_bytes = 1280;                     // >= (Cmax/16)*64 + 64 for Cmax = 256... host-checked below
    const int stat_bytes = 1024 + 64;                         // GN op scratch [S][2 x 32] overlaid with the fused-GroupNorm partial-sum slots (never live together)
    b.arena_init(TAB_RESERVE + zero_bytes + stat_bytes);
    b.gn_slot_off = TAB_RESERVE + zero_bytes;
    b.gn_fuse = std::getenv("RDMI_NO_GNFUSE") == nullptr;
    const int H0 = c->H, W0 = c->W;
    if (H0 * W0 > 96) { q.why = "more than 96 pixels per sample"; return 0; }
    const int nlev = a.n_levels, nrb = a.num_res_blocks;
    const bool multi = S > 1;
    size_t hand_down = 0, hand_up = 0;                // multi-sample: level-0 <-> low-resolution hand-off slots
    // ---- level 0, down path: once per sample slot (same LDS, same spill slots)
    for (int sl = 0; sl < nslot0; ++sl) {
        b.cur_samp = sl;
        b.slot_replay = sl > 0; b.slot_pos = 0;
        w.H = H0; w.W = W0; w.ch = a.nf;
        LT xin = b.talloc(16, H0, W0);
        b.gather_x(xin);
        w.h = b.talloc(a.nf, H0, W0);
        FusedBuilder::FConv in = b.conv_of("input_conv", ".bias", a.nf);
        in.in = &xin; in.dst = &w.h; in.stash = "input_conv";
        b.conv(in);
        b.tfree(xin);
        if (sl == 0) w.hs.push_back({(size_t)-1, a.nf, H0, W0});          // hs[0] (input_conv output) is never popped (RD/models/ncsnpp.py:268,315)
        for (int j = 0; j < nrb; ++j) w.down_block(j, sl == 0);
        if (sl == 0) w.hs.push_back(w.hs.back());
        if (nlev > 1) {
            w.downsample(0);
            if (multi && !coop) { hand_down = b.spill_store(w.h); b.tfree(w.h); }
        }
    }
    b.slot_replay = false;
    // ---- levels >= 1 (down), bottleneck, levels >= 1 (up): all S samples at once when S > 1.
    //      Co-operative program: only the levels of at most 4 pixels per sample (and the bottleneck) run in the shared form -- that
    //      part is bound by the weight stream and by 4-row MFMA tiles with one sample per CU; the 4x4 level is matrix-pipe bound
    //      either way (measured: sharing it costs more in exchanges than it saves) and stays per sample like level 0.
    int u = 0, loadtab_op = -1;
    {
        b.cur_samp = (multi && !coop) ? -1 : 0;
        bool in_coop = false;
        auto enter_multi = [&]() {
            b.multi_slot_off = b.alloc_top(4096);
            b.tab1_lds = b.alloc_top(TAB1_RESERVE);
            FOp lt = b.blank(FOP_LOADTAB);            // the section's row tables: global -> LDS (source / size patched below)
            lt.dst_off = b.tab1_lds;
            loadtab_op = b.emit(lt);
        };
        auto leave_multi = [&]() {
            b.free_bytes(b.multi_slot_off, 4096);
            b.multi_slot_off = -1;
            b.free_bytes(b.tab1_lds, TAB1_RESERVE);
            while (b.tabs1.size() % 8) b.tabs1.push_back(-1);
            q.fprog[(size_t)loadtab_op].rows = (int)b.tabs1.size() * 2;      // bytes
        };
        auto enter_coop = [&]() {                     // h: this member's own sample -> the four samples of the group (rows of sample m come from member m)
            b.flush_xchg();
            b.cur_samp = -1;
            enter_multi();
            LT h4 = b.talloc(w.ch, w.H, w.W);
            b.emit_xchg(h4, &w.h);
            b.tfree(w.h);
            w.h = h4; in_coop = true;
        };
        auto leave_coop = [&]() {                     // back to the member's own sample: its rows of the complete four-sample tensor
            b.flush_xchg();
            b.cur_samp = 0;
            LT own = b.talloc(w.ch, w.H, w.W);
            b.copy_t(own, w.h);
            q.fprog.back().a_hw = own.hw(); q.fprog.back().a_mstride = own.hw() * w.h.rs * 4;
            b.tfree(w.h);
            w.h = own; in_coop = false;
            leave_multi();
        };
        if (multi && !coop) {
            enter_multi();
            w.h = b.talloc(w.ch, w.H, w.W);
            b.gather_g(w.h, hand_down);
        }
        int coop_level = -1, d = nrb;
        for (int i = 1; i < nlev; ++i) {
            if (coop && !in_coop && w.H * w.W == 4) { enter_coop(); coop_level = i; }       // 4 pixels per sample: 4 samples = one 16-row MFMA tile
            for (int j = 0; j < nrb; ++j, ++d) w.down_block(d, true);
            w.hs.push_back(w.hs.back());
            if (i != nlev - 1) w.downsample(i);
        }
        if (coop && !in_coop) b.fail_("no level of exactly 4 pixels per sample: nothing to share");
        w.h = fused_resblock(b, "mid_block1", w.h, w.ch, w.dense_off.at("mid_block1"));
        w.h = fused_resblock(b, "mid_block2", w.h, w.ch, w.dense_off.at("mid_block2"));
        for (int k = 0; k < nlev - 1; ++k) {          // up levels nlev-1 .. 1
            for (int j = 0; j < nrb + 1; ++j, ++u) w.up_block(u);
            if (in_coop && nlev - 1 - k == coop_level) leave_coop();      // the levels above run per sample again
            if (k != nlev - 2) w.upsample(k);          // an upsample between two low levels stays in this section
        }
        if (in_coop) leave_coop();
        if (multi && !coop) {
            hand_up = b.spill_store(w.h); b.tfree(w.h);
            leave_multi();
        }
    }
    // ---- level 0, up path: once per sample slot
    const int ch_low = w.ch, H_low = w.H, W_low = w.W;
    const std::vector<FusedWalk::HS> hs0 = w.hs;
    for (int sl = 0; sl < nslot0; ++sl) {
        b.cur_samp = sl;
        w.ch = ch_low; w.H = H_low; w.W = W_low; w.hs = hs0;
        if (multi && !coop) { w.h = b.talloc(w.ch, w.H, w.W); b.gather_g(w.h, hand_up); }
        if (nlev > 1) w.upsample(nlev - 2);            // onto level 0's (even) grid
        for (int j = 0; j < nrb + 1; ++j) w.up_block(u + j);
        b.gn(w.h, "out_norm", true);
        FusedBuilder::FConv out = b.conv_of("out_conv", ".bias", a.channels);
        out.in = &w.h; out.dst_kind = 2;
        b.conv(out);
        b.tfree(w.h);
    }
    if (w.H != c->H || w.W != c->W) b.fail_("network output grid differs from the input grid");

    *tab_used = (int)q.ftabs.size() * 2 + 16;
    *tab1_used = (int)b.tabs1.size() * 2 + 16;
    if (*tab_used > TAB_RESERVE && TAB_RESERVE != 8 * 1024) b.fail_("row tables exceed the reserved LDS region");
    if (*tab1_used > TAB1_RESERVE && multi) b.fail_("low-resolution row tables exceed their LDS block");
    int cmax = 16;
    for (auto& o : q.fprog) if (o.kind == FOP_CONV) cmax = std::max(cmax, o.main_ph.nch * 16);
    if (cmax * 4 + 64 > zero_bytes) b.fail_("zero row too small");
    b.check_gn_slots();
    if (b.failed && TAB_RESERVE == 8 * 1024 && *tab_used <= 8 * 1024) return 0;      // pass 1 only sizes the tables
    if (b.failed) { q.why = b.why; return 0; }

    // table offsets (shorts, relative) -> LDS byte offsets
    auto tab_lds = [&](int ref) { return (ref >> 24) ? b.tab1_lds + (ref & 0xffffff) * 2 : (ref & 0xffffff) * 2; };
    for (auto& o : q.fprog) {
        if (o.kind == FOP_CONV) for (int t = 0; t < o.ntap; ++t) o.tab_off[t] = tab_lds(o.tab_off[t]);
        else if (o.kind == FOP_GATHER && o.a_map_off >= 0) o.a_map_off = tab_lds(o.a_map_off);
    }
    while (q.ftabs.size() % 8) q.ftabs.push_back(-1);
    const size_t tab0_shorts = q.ftabs.size();                  // region 0 is what the kernel copies at start; region 1 follows it in the buffer
    q.ftabs.insert(q.ftabs.end(), b.tabs1.begin(), b.tabs1.end());
    q.spill_per_sample = b.spill_floats;
    // spill slots are [slot][n][rows][C].  Co-operative program: the low-resolution slots are indexed by (workgroup, sample of its group),
    // n = 4 * workgroup id + slot, so the buffer holds 4 * (largest grid) "samples" per slot
    FusedPlan& plan = *c->fused;
    int coop_max_nb = 0, spill_n = c->max_batch;
    if (coop) {
        const int st = plan.coop_stride, res = resident_workgroups();
        const int max_groups = (res / (4 * st)) * st;                      // whole blocks of 4 * stride workgroup ids that are resident together
        coop_max_nb = std::min(c->max_batch, 4 * max_groups);
        if (coop_max_nb < 1) b.fail_("no room for one co-operative group");
        const int grid_max = ceil_div(ceil_div(std::max(coop_max_nb, 1), 4), st) * 4 * st;
        spill_n = 4 * grid_max;
    }
    if (b.failed) { q.why = b.why; return 0; }
    HIP_OK(hip_alloc(q.d_spill, std::max<size_t>(q.spill_per_sample, 1) * (size_t)spill_n));
    HIP_OK(hip_alloc(q.d_fprog, q.fprog.size()));
    HIP_OK(hip_alloc(q.d_ftabs, q.ftabs.size()));
    HIP_OK(hipMemcpy(q.d_ftabs.get(), q.ftabs.data(), q.ftabs.size() * sizeof(short), hipMemcpyHostToDevice));
    // spill slots: [slot][n][rows][C] so a workgroup only ever touches its own sample's rows
    for (auto& f : b.spill_fix) {
        FOp& o = q.fprog[(size_t)f.op];
        float* p = q.d_spill.get() + f.off * (size_t)spill_n;
        if (f.which == 1) o.b_g = p; else if (f.which == 2) o.a_g = p; else o.g_out = p;
    }
    UnetArgs& fa = q.fargs;
    fa = UnetArgs{};
    fa.prog = q.d_fprog.get(); fa.nops = (int)q.fprog.size();
    fa.tabs = q.d_ftabs.get(); fa.tab_bytes = (int)(tab0_shorts * sizeof(short)); fa.tab_base = 0;
    if (loadtab_op >= 0) q.fprog[(size_t)loadtab_op].a_g = reinterpret_cast<const float*>(q.d_ftabs.get() + tab0_shorts);
    fa.zero_off = TAB_RESERVE; fa.zero_bytes = zero_bytes;
    fa.dense = c->d_dense.get(); fa.dense_stride = c->dense_total; fa.S = S;
    fa.out_elems = c->H * c->W * a.channels;
    if (coop) {
        const int groups_max = ceil_div(coop_max_nb, 4);
        const size_t xb = (size_t)groups_max * 2 * 4 * (size_t)b.xslot_granules * sizeof(unsigned long long);
        HIP_OK(hip_alloc(q.d_xbuf, std::max<size_t>(xb, 16) / sizeof(unsigned long long)));
        HIP_OK(hipMemset(q.d_xbuf.get(), 0, std::max<size_t>(xb, 16)));          // tags start at 0; epochs never are
        HIP_OK(hip_alloc(q.d_coop_err, 4));
        HIP_OK(hipMemset(q.d_coop_err.get(), 0, 16));
        fa.coop = 1; fa.coop_stride = plan.coop_stride; fa.xbuf = q.d_xbuf.get(); fa.xslot = b.xslot_granules;
        fa.coop_err = q.d_coop_err.get();
        if (const char* e = std::getenv("RDMI_COOP_TEST_BREAK")) fa.coop_break = atoi(e);
        q.coop = true; q.n_xchg = b.n_xchg; q.max_nb = coop_max_nb;
    }
    q.fused_lds = (size_t)b.high_water;
    if (const char* e = std::getenv("RDMI_UDBG")) fa.dbg = atoi(e);
    if (std::getenv("RDMI_STAMPS") && (S == 1 || coop)) {       // diagnostic builds exist for the single-sample and the co-operative program
        if (!plan.d_stamps) HIP_OK(hip_alloc(plan.d_stamps, 1024 + 200 * 8 + 8));
        if (q.fprog.size() > 200) return fail("RDMI_STAMPS: program of %zu ops", q.fprog.size());
        fa.stamps = plan.d_stamps.get();
    }
    q.fdesc.clear();
    for (auto& o : q.fprog) {
        char buf[160];
        const char* kn[] = {"GATHER", "STORE", "GN", "CONV", "ATTN", "LOADTAB", "XCHG"};
        if (o.kind == FOP_CONV) snprintf(buf, sizeof buf, "CONV rows=%d mtiles=%d K=%dx%d(+%d) Cout=%d dst=%d%s", o.rows, o.mtiles, o.ntap, o.main_ph.nch * 16, 0, o.Cout, o.dst_kind, o.gn_off >= 0 ? (o.gn_raw ? (o.coop ? " +GN(copy) coop" : " +GN(copy)") : (o.coop ? " +GN coop" : " +GN")) : (o.coop ? " coop" : ""));
        else snprintf(buf, sizeof buf, "%s rows=%d C=%d", kn[o.kind], o.rows, o.C);
        q.fdesc.push_back(buf);
    }
    q.ok = true;
    return 0;
}

// Two passes: the first sizes the row-table regions (and is dropped), the second builds the program with them sized exactly.
int build_one_program(rdmi_ctx* c, int S, bool coop = false, bool train = false) {
    int used = 0, used1 = 0;
    {
        FusedProg sizing;
        if (int e = build_fused_program_pass(c, sizing, S, 8 * 1024, 24 * 1024, &used, &used1, coop, train)) return e;
    }
    FusedProg q;
    if (int e = build_fused_program_pass(c, q, S, (used + 63) & ~63, (used1 + 63) & ~63, &used, &used1, coop, train)) return e;
    c->fused->progs.push_back(std::move(q));
    return 0;
}

int build_fused_program(rdmi_ctx* c, const std::map<std::string, int>& dense_off) {
    c->fused = std::make_unique<FusedPlan>();
    FusedPlan& plan = *c->fused;
    plan.dense_off = dense_off;
    // S = 1: one sample per workgroup (B <= 128 with guidance fills the 256 CUs exactly).  Larger batches run the
    // low-resolution half of the network for S = 2 / 4 samples at once per workgroup: every streamed weight fragment then
    // feeds S samples (that half is weight-stream bound at S = 1) and its per-op fixed cost is shared.
    if (int e = build_one_program(c, 1)) return e;
    const char* only = std::getenv("RDMI_S");           // RDMI_S=1 keeps the single-sample program only (A/B)
    if (const char* e = std::getenv("RDMI_S_MIN_WG")) plan.s_min_wg = std::max(1, atoi(e));
    for (int S : {2, 4})
        if (plan.progs[0].ok && c->arch.n_levels >= 2 && c->max_batch >= plan.s_min_wg * S && (!only || atoi(only) >= S))
            if (int e = build_one_program(c, S)) return e;
    // The co-operative program (groups of four workgroups share the low-resolution section): for batches that fit the chip in one
    // wave of workgroups.  RDMI_COOP=0 leaves it out; RDMI_COOP_STRIDE sets the distance between a group's workgroup ids.
    if (const char* e = std::getenv("RDMI_COOP")) plan.use_coop = atoi(e) != 0;
#ifdef RDMI_EMU
    plan.coop_stride = 1;          // the emulator runs consecutive workgroup ids concurrently
#endif
    if (const char* e = std::getenv("RDMI_COOP_STRIDE")) plan.coop_stride = std::max(1, atoi(e));
    if (plan.progs[0].ok && plan.use_coop && c->arch.n_levels >= 2 && !only)
        if (int e = build_one_program(c, 4, true)) return e;
    return 0;
}

// Parameter-dependent pointers of a program's descriptors (from the bound parameters and the weight arena), then the upload.
int bind_fused_params(rdmi_ctx* c, FusedProg& q, hipStream_t s) {
    for (const FPatch& f : q.fpatch) {
        FOp& o = q.fprog[(size_t)f.op];
        const float* p = f.param < 0 ? c->d_w.get() + f.arena_off : c->params[(size_t)f.param].ptr;
        switch (f.field) {
            case F_GAMMA: o.gamma = p; break;
            case F_BETA: o.beta = p; break;
            case F_BIAS: o.bias = p; break;
            case F_W: o.main_ph.w = p; break;
        }
    }
    HIP_OK(hipMemcpyAsync(q.d_fprog.get(), q.fprog.data(), q.fprog.size() * sizeof(FOp), hipMemcpyHostToDevice, s));
    return 0;
}

// One workgroup-resident launch of program q over the batch of f.
int run_fused(rdmi_ctx* c, const FusedProg& q, const FwdIn& f, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set) {       // every instantiation a program can ask for (<diagnostic, multi-sample, co-operative, training>)
        const void* ks[] = {(const void*)unet_wg_kernel<false>, (const void*)unet_wg_kernel<true>, (const void*)unet_wg_kernel<false, true>, (const void*)unet_wg_kernel<false, true, true>,
                            (const void*)unet_wg_kernel<true, true, true>, (const void*)unet_wg_kernel<false, false, false, true>};
        for (const void* k : ks) HIP_OK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    FusedPlan& plan = *c->fused;
    UnetArgs ua = q.fargs;
    ua.x_in = f.x; ua.x_mod = f.x_mod; ua.out = f.out; ua.NB = f.NB;
    unsigned nwg = (unsigned)ceil_div(f.NB, q.S);
    if (q.coop) {          // groups of four workgroups, whole blocks of 4 * stride ids; every launch gets fresh exchange tags
        nwg = (unsigned)(ceil_div(ceil_div(f.NB, 4), ua.coop_stride) * 4 * ua.coop_stride);
        ua.epoch_base = plan.coop_epoch;
        plan.coop_epoch += (unsigned)q.n_xchg;
        if (plan.coop_epoch > 0xfff00000u) plan.coop_epoch = 0;        // tags only have to differ from the two previous uses of a slot
    }
    if (f.dense_rows) ua.dense = f.dense_rows;
    double fl = 0;
    for (auto& op : c->ops) fl += op.flops_per_sample;
    ProfScope ps(c, s, "unet_wg_kernel", fl * f.NB);
    plan.last_prog = (int)(&q - plan.progs.data());
    const dim3 grid(nwg), block(UW_THREADS);
    if (q.train) {
        ua.drop_p = c->train_drop_p; ua.seed_dev = c->train_seed_dev;
        hipLaunchKernelGGL((unet_wg_kernel<false, false, false, true>), grid, block, q.fused_lds, s, ua);
    }
    else if ((ua.stamps || ua.dbg) && q.S == 1) hipLaunchKernelGGL(unet_wg_kernel<true>, grid, block, q.fused_lds, s, ua);   // diagnostic build
    else if ((ua.stamps || ua.dbg) && q.coop) hipLaunchKernelGGL((unet_wg_kernel<true, true, true>), grid, block, q.fused_lds, s, ua);
    else if (q.coop) hipLaunchKernelGGL((unet_wg_kernel<false, true, true>), grid, block, q.fused_lds, s, ua);
    else if (q.S > 1) hipLaunchKernelGGL((unet_wg_kernel<false, true>), grid, block, q.fused_lds, s, ua);
    else hipLaunchKernelGGL(unet_wg_kernel<false>, grid, block, q.fused_lds, s, ua);
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace
