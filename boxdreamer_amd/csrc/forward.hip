// Whole-path entry points: the DINOv2 encoder (DinoV2Wrapper.predict) and the BETR decoder
// (BETR.forward) as straight-line sequences of kernel launches on the caller's stream.
// No device allocation, no synchronisation, no state: the caller provides one workspace blob that is
// carved here (256-byte aligned slices).
#include <vector>

#include "bd_common.h"

namespace {

struct Carver {
    unsigned char* base;
    size_t off;
    void* take(size_t bytes) {
        off = (off + 255) & ~(size_t)255;
        void* p = base ? base + off : nullptr;
        off += bytes;
        return p;
    }
};

inline int planes_of(int prec) {      // 2-byte units per element of a 16-bit operand buffer (F16C8: f16 plane + e4m3 plane)
    return (prec == BD_PREC_BF16X3 || prec == BD_PREC_BF16X3_ATTN_X3 || prec == BD_PREC_F16C8 || prec == BD_PREC_F16C8_QK16 ||
            prec == BD_PREC_F16X3 || prec == BD_PREC_F16X3_ATTN_X3) ? 2 : 1;
}

struct BlockBufs {
    float* x;        // fp32 residual stream [M, D]
    void* xn;        // 16-bit LN output     [M, D]
    void* qkv;       // 16-bit               [M, 3D]
    void* ao;        // 16-bit attention out [M, D]
    void* h;         // 16-bit MLP hidden    [M, 4D]
    float* st;       // LayerNorm fold: (mean, M2) per row and 96-column group [M, D / 96, 2] fp32 (F16C8 family)
    void* sk;        // split-K scratch of the residual Linears (bd_gemm_args.sk_ws; small M only, else NULL); flags zeroed per forward
    size_t sk_flag_bytes;
};

inline bd_gemm_args gemm_args(const void* A, int64_t lda, int64_t a_plane, const bd_linear& lin, int64_t ldw, int N,
                              void* out, int64_t ldo, int64_t out_plane, int out_f32, int M, int K, int act) {
    bd_gemm_args g{};
    g.A = A; g.lda = lda; g.a_plane = a_plane;
    g.W = lin.w; g.ldw = ldw; g.w_plane = (int64_t)N * ldw;
    g.bias = lin.b;
    g.wscale = lin.wscale;
    g.out = out; g.ldo = ldo; g.out_plane = out_plane; g.out_f32 = out_f32;
    g.M = M; g.N = N; g.K = K; g.act = act;
    g.w_qexp = lin.w_qexp;
    return g;
}

#define BD_TRY(expr) do { int rc__ = (expr); if (rc__ != BD_OK) return rc__; } while (0)

// Attention policy of the strict (split-bf16 x3) family.  The variants are separate `prec` values of the whole-path
// entry points (no environment switches, no library state):
//   BD_PREC_BF16X3           GEMMs split-bf16; attention as ONE f16 pass where q and k are RMS-normalised (BETR: the x3 QKV
//                            GEMM stores q, k, v as a single f16 plane, q/k RMSNorm and attention run in f16, attention writes
//                            (hi, lo) bf16 planes for the x3 proj GEMM); DINOv2's attention (un-normalised q.k) stays
//                            split-bf16.  Measured 1.3e-4 on the logits at full depth, T = 6.
//   BD_PREC_BF16X3_ATTN_X3   split-bf16 attention everywhere (8.2e-5, ~8 % slower)
// (f16 attention everywhere -- ABI <= 6's BD_PREC_BF16X3_ATTN_F16 -- measured 1.18e-3: the f16 Q.K^T on DINOv2's un-normalised
// q / k eats the whole budget; removed in ABI 7.)
inline int gemm_prec(int prec) {
    if (prec == BD_PREC_F16C8_QK16) return BD_PREC_F16C8;
    if (prec == BD_PREC_F16X3_ATTN_X3) return BD_PREC_F16X3;
    return prec == BD_PREC_BF16X3_ATTN_X3 ? BD_PREC_BF16X3 : prec;
}
inline bool qk_single_f16(int prec) { return prec == BD_PREC_F16C8_QK16; }
inline bool x3_f16_attention(int prec, bool qk_normed) { return (prec == BD_PREC_BF16X3 || prec == BD_PREC_F16X3) && qk_normed; }
inline bool split16(int cls) { return cls == BD_PREC_BF16X3 || cls == BD_PREC_F16X3; }
// operand class of a Linear whose BD_PROMOTE_* bit is set (include/boxdreamer_hip.h): F16C8 family -> split-f16, e4m3 -> bf16
inline int promoted_class(int base) { return base == BD_PREC_F16C8 ? BD_PREC_F16X3 : (base == BD_PREC_FP8 ? BD_PREC_BF16 : base); }
inline int lin_class(int base, int promote, int bit) { return (promote & bit) ? promoted_class(base) : base; }
// fc1 -> fc2 and adapter fc1 -> fc2 hand-offs: a promoted GEMM cannot emit the base operand class, so promoting the first promotes the second
inline int norm_promote(int pm) { return (pm & BD_PROMOTE_FC1) ? (pm | BD_PROMOTE_FC2) : pm; }
// output kind (bd_gemm_args.out_f32) with which a GEMM of class `from` writes the A operand of a Linear of class `to`
inline int handoff_kind(int from, int to) {
    return from == to ? 0 : (to == BD_PREC_BF16 ? 3 /* e4m3 GEMM -> bf16 plane */ : 5 /* F16C8 GEMM -> split-f16 planes */);
}

// One transformer stack of one call: its weights, buffers and geometry (M = batch x seq rows of the residual stream).
struct Stack {
    const bd_block_weights* blocks;
    int depth, M, batch, seq, D, heads;
    float ln_eps, rms_eps;
    BlockBufs b;
    bool lat;                        // latency forms (bd_betr_weights.latency_mode at one or two poses): attention's, and the QK16 swap (plan_stack)
    int n_prefix;                    // DINOv2: cls + registers lead every image's tokens
    const int32_t* query_idx;        // BETR: the last block runs the query view's P rows per sample past K / V ...
    int P;
    float* xc;                       // ... on this compact fp32 stream [batch * P, D]
    // Ragged batch (bd_decoder_forward_ragged): sample b owns the views [view_start[b], view_start[b + 1]) of the packed stream, M = n_views * P
    // rows; query_idx counts inside the sample.  Only attention and the query-row gather know where a sample starts (run_block).
    const int32_t* view_start;       // device int32 [batch + 1], or NULL: every sample has seq rows
    int n_views, max_views;
};

// Attention forms.  PREFIX_SKIP (last DINOv2 block): the prefix rows are never read again, so their attention is skipped
// (bd_attention_prefix) -- proj and the MLP then run on stale attention rows there, whose results nobody consumes (row-wise operators:
// nothing leaks into the patch rows).  QUERY_ONLY (last BETR block): its output is consumed for the query view only (betr.py:303), so
// only K / V need every token: LN1 + QKV (+ q/k RMSNorm) run on all rows, attention takes queries from the query view's P rows and
// writes a compact [B*P, D] result, proj, LN2 and the MLP run on those B*P rows (1/T of the work).  Row-wise arithmetic is unchanged,
// so the result is bit-identical to the full-width block.
enum { ATTN_FULL, ATTN_PREFIX_SKIP, ATTN_QUERY_ONLY };

// How one transformer block runs: its entry in the stack's schedule (plan_stack), complete before the first launch of the call.
struct BlockPlan {
    const bd_block_weights* w;
    int prec;                        // the block's precision (wprec after the latency-forms swap)
    int base;                        // operand class of the un-promoted Linears
    int c_qkv, c_proj, c_fc1, c_fc2; // operand class per Linear (F16C8 family: per-Linear promotion to split-f16; e4m3: to bf16)
    bool hyb;                        // attention as ONE f16 pass on a single f16 q, k, v plane (q, k RMS-normalised)
    bool qk16;                       // BETR's QKV Linear split by column (q, k one f16 pass on the f16 plane, v the full F16C8 product)
    int qkv_out;                     // output kind of the QKV GEMM
    int aprec_in;                    // class of the attention input (for the stand-alone q/k RMSNorm)
    int aprec;                       // bd_attention precision code (input form x class of proj's A operand)
    int attn;                        // ATTN_*
    int Mr;                          // rows of the residual side: the stream's M, or the query view's B*P rows (ATTN_QUERY_ONLY)
    float* x;                        // fp32 stream of the residual side: BlockBufs.x, or Stack.xc
    bool rms_fused;                  // q/k RMSNorm in the QKV launch's epilogue
    bool ln1_folded;                 // LayerNorm 1 folded behind the previous block's fc2
    bool emit_next;                  // fc2 emits the operand copy / row statistics for the next block's folded LayerNorm 1
    bool fold2;                      // LayerNorm 2 folded between proj and fc1
    bool proj_c8, proj_f32, fc2_c8, fc2_f32;    // the 3-byte residual stream (plan_resid)
    bool sk;                         // split-K scratch lent to proj and fc2
};
inline BlockPlan plan_block(const bd_block_weights& w, int wprec) {
    BlockPlan p{};
    p.w = &w;
    p.prec = wprec;
    p.base = gemm_prec(wprec);
    const bool c8 = p.base == BD_PREC_F16C8, f8 = p.base == BD_PREC_FP8, normed = w.q_norm_w != nullptr;
    const int pm = (c8 || f8) ? norm_promote(w.promote) : 0;
    p.c_qkv = lin_class(p.base, pm, BD_PROMOTE_QKV);
    p.c_proj = lin_class(p.base, pm, BD_PROMOTE_PROJ);
    p.c_fc1 = lin_class(p.base, pm, BD_PROMOTE_FC1);
    p.c_fc2 = lin_class(p.base, pm, BD_PROMOTE_FC2);
    p.hyb = (split16(p.base) && x3_f16_attention(wprec, normed)) || (c8 && normed && !(pm & BD_PROMOTE_ATTN));
    const bool plain_qkv = p.c_qkv == p.base;          // the special QKV forms exist for the un-promoted Linear only
    p.qk16 = qk_single_f16(wprec) && p.hyb && w.qkv16.w && plain_qkv;
    if (p.hyb) { p.qkv_out = 2; p.aprec_in = BD_PREC_F16; }                                  // one f16 plane
    else if (f8) { p.qkv_out = p.c_qkv == BD_PREC_FP8 ? 3 : 0; p.aprec_in = BD_PREC_BF16; }   // one bf16 plane (an e4m3 or a bf16 GEMM's)
    else if (p.c_qkv == BD_PREC_F16C8 || p.c_qkv == BD_PREC_F16X3) { p.qkv_out = 4; p.aprec_in = BD_PREC_BF16X3; }   // split-bf16 planes for
                                                                                              // the split-bf16 attention (range: probabilities)
    else { p.qkv_out = 0; p.aprec_in = p.c_qkv; }                                             // the GEMM's own operand class
    if (p.hyb) p.aprec = p.c_proj == BD_PREC_F16C8 ? BD_PREC_F16_OUT_F16C8 : (p.c_proj == BD_PREC_F16X3 ? BD_PREC_F16_OUT_F16X3 : BD_PREC_F16_OUT_BF16X3);
    else if (f8) p.aprec = p.c_proj == BD_PREC_FP8 ? BD_PREC_BF16_OUT_FP8 : BD_PREC_BF16;
    else if (p.aprec_in == BD_PREC_BF16X3)
        p.aprec = p.c_proj == BD_PREC_F16C8 ? BD_PREC_BF16X3_OUT_F16C8 : (p.c_proj == BD_PREC_F16X3 ? BD_PREC_BF16X3_OUT_F16X3 : BD_PREC_BF16X3);
    else p.aprec = p.base;
    return p;
}

// ---- The Linear launches of a block, built from its schedule entry.  The planner hands candidate entries to bd_gemm_takes_ln_fold /
// bd_gemm_fuses_qk_rmsnorm, run_block hands the final entry to bd_gemm: both see the same arguments.
struct Lin { bd_gemm_args g; int cls; };
inline int launch(const Lin& l, void* stream) { return bd_gemm(&l.g, l.cls, stream); }
inline bool takes_fold(const Lin& l) { return bd_gemm_takes_ln_fold(&l.g, l.cls) != 0; }
inline void ln_consumer(bd_gemm_args& g, const BlockBufs& b, const float* colsum, float eps) { g.ln_stats_in = b.st; g.ln_colsum = colsum; g.ln_eps = eps; }

// The QKV Linear on the stream's M rows, leaving q, k, v in b.qkv in the form the entry's attention reads.
// BD_PREC_F16C8_QK16: the QKV Linear of a block whose q, k are RMS-normalised, split by output column (include/boxdreamer_hip.h):
// LayerNorm 1 emits the F16C8 operand; launch 1 (this one) multiplies its f16 plane with the f16 copy of the q, k weight rows (one MFMA
// pass), launch 2 (qk16_v_lin) is the full F16C8 product for the v rows.  q, k, v land in one f16 [M, 3D] buffer exactly as the
// single-launch forms lay them out.
Lin qkv_lin(const BlockPlan& e, const Stack& s) {
    const bd_block_weights& w = *e.w;
    const int D = s.D;
    const int64_t pD = (int64_t)s.M * D;
    Lin l;
    if (e.qk16) {      // rows [0, 2D) of the f16 copy
        l = {gemm_args(s.b.xn, D, 0, e.ln1_folded ? w.qkv16_f : w.qkv16, D, 2 * D, s.b.qkv, 3 * D, 0, 0, s.M, D, BD_ACT_NONE), BD_PREC_F16};
        if (e.rms_fused) l.g.rms_parts = 2;
    } else
        l = {gemm_args(s.b.xn, D, pD, e.ln1_folded ? w.qkv_f : w.qkv, D, 3 * D, s.b.qkv, 3 * D, 3 * pD, e.qkv_out, s.M, D, BD_ACT_NONE), e.c_qkv};
    if (e.rms_fused) { l.g.rms_wq = w.q_norm_w; l.g.rms_wk = w.k_norm_w; l.g.rms_eps = s.rms_eps; }
    if (e.ln1_folded) ln_consumer(l.g, s.b, e.qk16 ? w.qkv16_s : w.qkv_s, s.ln_eps);
    return l;
}
Lin qk16_v_lin(const BlockPlan& e, const Stack& s) {
    const int D = s.D;
    bd_linear v = e.ln1_folded ? e.w->qkv_f : e.w->qkv;       // rows [2D, 3D) of the F16C8 weight: both planes advance by 2D rows
    v.w = (const unsigned short*)v.w + (int64_t)2 * D * D;
    v.b = v.b + 2 * D;
    Lin l{gemm_args(s.b.xn, D, (int64_t)s.M * D, v, D, D, (unsigned short*)s.b.qkv + 2 * D, 3 * D, 0, 2 /* f16 plane */, s.M, D, BD_ACT_NONE),
          BD_PREC_F16C8};
    l.g.w_plane = (int64_t)3 * D * D;                           // plane 1 still lies one FULL weight plane behind plane 0
    if (e.ln1_folded) ln_consumer(l.g, s.b, e.w->qkv_s + 2 * D, s.ln_eps);
    return l;
}
// does the QKV launch of this entry take the q/k RMSNorm into its epilogue?
inline bool qkv_fuses_rms(BlockPlan e, const Stack& s) {
    e.rms_fused = true;
    const Lin l = qkv_lin(e, s);
    return bd_gemm_fuses_qk_rmsnorm(&l.g, l.cls) != 0;
}

// A residual Linear (proj, fc2): e.x += A W^T + b on e.Mr rows.  LayerNorm fold, producer side: the epilogue also emits the raw row as
// the F16C8 operand (b.xn) + its row statistics (b.st) for the LayerNorm behind it.  from_copy (3-byte stream): the residual rows are
// read from that operand copy and the sum is written back there, as fp32 rows too only if f32_too.
// Split-K scratch: lent on at most as many rows as the region was carved for (the stream's M; the last decoder block's compact rows are fewer).
Lin resid_lin(const BlockPlan& e, const Stack& s, const void* A, const bd_linear& lin, int K, int cls, bool emit, bool from_copy, bool f32_too) {
    const int D = s.D;
    Lin l{gemm_args(A, K, (int64_t)e.Mr * K, lin, K, D, e.x, D, 0, 1, e.Mr, K, BD_ACT_NONE), cls};
    l.g.resid = e.x; l.g.ldr = D;
    if (e.sk) l.g.sk_ws = s.b.sk;
    if (emit || from_copy) { l.g.ln_stats_out = s.b.st; l.g.ln_op_out = s.b.xn; l.g.ln_op_plane = (int64_t)e.Mr * D; l.g.ln_op_ld = D; }
    if (from_copy) { l.g.ln_resid_in_op = 1; l.g.resid = nullptr; l.g.ldr = 0; l.g.out_f32 = f32_too ? 1 : 0; }
    return l;
}
Lin proj_lin(const BlockPlan& e, const Stack& s) { return resid_lin(e, s, s.b.ao, e.w->proj, s.D, e.c_proj, e.fold2, e.proj_c8, e.proj_f32); }
Lin fc2_lin(const BlockPlan& e, const Stack& s) { return resid_lin(e, s, s.b.h, e.w->fc2, 4 * s.D, e.c_fc2, e.emit_next, e.fc2_c8, e.fc2_f32); }
Lin fc1_lin(const BlockPlan& e, const Stack& s) {
    const int D = s.D;
    Lin l{gemm_args(s.b.xn, D, (int64_t)e.Mr * D, e.fold2 ? e.w->fc1_f : e.w->fc1, D, 4 * D, s.b.h, 4 * D, (int64_t)e.Mr * 4 * D,
                    handoff_kind(e.c_fc1, e.c_fc2), e.Mr, D, BD_ACT_GELU), e.c_fc1};
    if (e.fold2) ln_consumer(l.g, s.b, e.w->fc1_s, s.ln_eps);
    return l;
}

// ---- The 3-byte residual stream (bd_gemm_args.ln_resid_in_op, bd_block_weights.ln_resid3): between FOLDED LayerNorms nobody reads the
// stream as fp32 -- the next reader is a Linear that multiplies the operand copy -- so a residual Linear may read its residual rows from
// that copy (b.xn) and write the sum back there only.  What decides, per residual Linear:
//   reads the copy   iff b.xn IS the stream (the LayerNorm in front of it was folded) and the launch has the form (un-promoted F16C8);
//   writes fp32 too  iff someone reads b.x before the next residual Linear: a LayerNorm kernel, a residual Linear without that form, the
//                    stack's final norm / the last decoder block's row gather.
// plan_resid decides the stream between block e and the block behind it (next; its LayerNorms are planned): whether next's proj reads
// the copy, whether e's fc2 writes the copy and whether fp32 rows too; e's proj writes fp32 rows unless e's fc2 reads the copy.
void plan_resid(BlockPlan& e, BlockPlan* next, const Stack& s) {
    if (next && next->ln1_folded && next->fold2 && next->x == s.b.x && next->w->ln_resid3) {
        BlockPlan c = *next;
        c.proj_c8 = true;
        next->proj_c8 = takes_fold(proj_lin(c, s));
    }
    if (e.fold2 && e.emit_next && e.w->ln_resid3) {
        BlockPlan c = e;
        c.fc2_c8 = true;
        e.fc2_c8 = takes_fold(fc2_lin(c, s));
    }
    e.proj_f32 = !e.fc2_c8;                  // (LayerNorm 2 as a kernel implies !fold2, hence !fc2_c8)
    e.fc2_f32 = !next || !next->proj_c8;
}

// ---- The schedule of a stack: one entry per block, every decision taken before the first launch.
// LayerNorm fold (ABI 8, include/boxdreamer_hip.h bd_gemm_args.ln_*): between a residual Linear (proj, fc2) and the Linear(s) behind the
// next LayerNorm (fc1; the next block's QKV) of the F16C8 family the LayerNorm launch is replaced by (a) the residual Linear's epilogue
// emitting the raw row as the F16C8 operand + per-wave-tile (mean, M2) pairs and (b) the consumer's epilogue applying the row statistics to a
// product with the gain-folded weight (bd_block_weights.qkv_f / fc1_f / qkv16_f).  A hand-off folds only when EVERY launch on both sides has a
// kernel form for it (bd_gemm_takes_ln_fold) -- un-promoted F16C8 Linears, D = 768; everything else keeps the bd_layernorm launch.  The
// first LayerNorm of a stack (no residual Linear in front of it) and the stacks' final norms stay kernels.
int plan_stack(const Stack& s, int wprec, std::vector<BlockPlan>& sched) {
    // (latency forms, one or two poses per call: the q, k / v column split of BD_PREC_F16C8_QK16 is two launches of ~20 us each where one
    // F16C8 QKV launch takes ~26 us -- at these sizes a launch costs its fixed part, not its passes; q, k then carry the full F16C8 product)
    const int bprec = (s.lat && wprec == BD_PREC_F16C8_QK16) ? BD_PREC_F16C8 : wprec;
    const int D = s.D;
    sched.assign(s.depth > 0 ? s.depth : 0, BlockPlan{});
    for (int i = 0; i < s.depth; ++i) {
        const bd_block_weights& w = s.blocks[i];
        BlockPlan& e = sched[i];
        BlockPlan* prev = i > 0 ? &sched[i - 1] : nullptr;
        e = plan_block(w, bprec);
        const bool last = i + 1 == s.depth;
        e.attn = !last ? ATTN_FULL : (s.query_idx ? ATTN_QUERY_ONLY : (s.n_prefix > 0 && s.seq > s.n_prefix ? ATTN_PREFIX_SKIP : ATTN_FULL));
        e.Mr = e.attn == ATTN_QUERY_ONLY ? s.batch * s.P : s.M;
        e.x = e.attn == ATTN_QUERY_ONLY ? s.xc : s.b.x;
        e.sk = s.b.sk && e.Mr <= BD_SPLITK_MAX_ROWS;
        // LayerNorm 1 folds behind the previous block's fc2 when both sides have the fold form; the q/k RMSNorm (head_dim 96) fuses
        // into the QKV launch where that launch, folded or not, allows it
        const bool rms = w.q_norm_w && D / s.heads == 96;
        if (prev && prev->c_fc2 == BD_PREC_F16C8 && e.c_qkv == BD_PREC_F16C8 && D == 768 && w.qkv_f.w && w.qkv_s &&
            (!e.qk16 || (w.qkv16_f.w && w.qkv16_s))) {
            BlockPlan c = e, cp = *prev;
            c.ln1_folded = cp.emit_next = true;
            c.rms_fused = rms && qkv_fuses_rms(c, s);
            if (takes_fold(fc2_lin(cp, s)) && takes_fold(qkv_lin(c, s)) && (!c.qk16 || takes_fold(qk16_v_lin(c, s)))) {
                e = c;
                prev->emit_next = true;
            }
        }
        if (!e.ln1_folded) e.rms_fused = rms && qkv_fuses_rms(e, s);
        // LayerNorm 2 folds between proj and fc1
        if (w.fc1_f.w && w.fc1_s && e.c_proj == BD_PREC_F16C8 && e.c_fc1 == BD_PREC_F16C8 && e.c_fc2 == BD_PREC_F16C8 && D == 768) {
            BlockPlan c = e;
            c.fold2 = true;
            e.fold2 = takes_fold(proj_lin(c, s)) && takes_fold(fc1_lin(c, s));
        }
        if (prev) plan_resid(*prev, &e, s);
    }
    if (s.depth > 0) plan_resid(sched.back(), nullptr, s);
    // b.x stale (the previous fc2 wrote the copy only) must meet a proj that reads the copy, and the stack must end with fp32 rows (final
    // norm, head gather): plan_resid looks ahead so that neither can fail, and a failure here enqueues nothing
    bool stale = false;
    for (const BlockPlan& e : sched) {
        if (stale && !e.proj_c8) return BD_ERR_SHAPE;
        stale = e.fc2_c8 && !e.fc2_f32;
    }
    return stale ? BD_ERR_SHAPE : BD_OK;
}

// One pre-LN transformer block as its entry says: x += proj(attn(LN1 x)); x += fc2(gelu(fc1(LN2 x))).
// BETR: blocks.py:876-886 (+ q/k RMSNorm :257); DINOv2: layers/block.py:89-114 (LayerScale folded).
int run_block(const BlockPlan& e, const Stack& s, void* stream) {
    const bd_block_weights& w = *e.w;
    const BlockBufs& b = s.b;
    const int D = s.D, hd = D / s.heads;
    const int64_t pD = (int64_t)s.M * D, rD = (int64_t)e.Mr * D;
    if (!e.ln1_folded) BD_TRY(bd_layernorm(b.x, D, w.ln1_w, w.ln1_b, s.ln_eps, b.xn, pD, nullptr, 0, s.M, D, 0, 0, 0, e.c_qkv, stream));
    BD_TRY(launch(qkv_lin(e, s), stream));
    if (e.qk16) BD_TRY(launch(qk16_v_lin(e, s), stream));
    if (w.q_norm_w && !e.rms_fused) BD_TRY(bd_qk_rmsnorm(b.qkv, 3 * pD, w.q_norm_w, w.k_norm_w, s.rms_eps, s.M, s.heads, hd, e.aprec_in, stream));
    const float scale = 1.0f / sqrtf((float)hd);
    const bool qo = e.attn == ATTN_QUERY_ONLY;
    if (s.view_start)
        BD_TRY(bd_attention_varlen(b.qkv, 3 * pD, b.ao, rD, s.view_start, s.batch, s.n_views, s.max_views, s.P, s.heads, hd, scale,
                                   qo ? s.query_idx : nullptr, e.aprec, stream));
    else if (e.attn == ATTN_PREFIX_SKIP)
        BD_TRY(bd_attention_prefix(b.qkv, 3 * pD, b.ao, pD, s.batch, s.seq, s.heads, hd, scale, s.n_prefix, 0, e.aprec, stream));
    else
        BD_TRY(bd_attention_q_forms(b.qkv, 3 * pD, b.ao, rD, s.batch, s.seq, s.heads, hd, scale, qo ? s.query_idx : nullptr, qo ? s.P : s.seq,
                                    e.aprec, s.lat ? 1 : 0, stream));
    if (qo && s.view_start) BD_TRY(bd_gather_query_rows_f32_varlen(b.x, s.view_start, s.query_idx, e.x, s.batch, s.P, D, stream));
    else if (qo) BD_TRY(bd_gather_query_rows_f32(b.x, s.query_idx, e.x, s.batch, s.seq / s.P, s.P, D, stream));
    BD_TRY(launch(proj_lin(e, s), stream));
    if (!e.fold2) BD_TRY(bd_layernorm(e.x, D, w.ln2_w, w.ln2_b, s.ln_eps, b.xn, rD, nullptr, 0, e.Mr, D, 0, 0, 0, e.c_fc1, stream));
    BD_TRY(launch(fc1_lin(e, s), stream));
    return launch(fc2_lin(e, s), stream);
}

BlockBufs carve_block(Carver& c, int64_t M, int D, int np, bool latency) {
    BlockBufs b;
    b.x = (float*)c.take((size_t)M * D * 4);
    b.xn = c.take((size_t)M * D * 2 * np);
    b.qkv = c.take((size_t)M * 3 * D * 2 * np);
    b.ao = c.take((size_t)M * D * 2 * np);
    b.h = c.take((size_t)M * 4 * D * 2 * np);
    b.st = (float*)c.take((size_t)M * ((D + 95) / 96) * 2 * 4);
    // split-K scratch for the stream's residual Linears when the caller opted into the latency forms (bd_*_weights.latency_mode) and the
    // whole stream is a few tiles (one or two poses at a time)
    const size_t skb = (latency && np == 2 && M <= BD_SPLITK_MAX_ROWS) ? bd_gemm_splitk_workspace_bytes((int)M, D) : 0;
    b.sk = skb ? c.take(skb) : nullptr;
    b.sk_flag_bytes = skb ? bd_gemm_splitk_flag_bytes((int)M, D) : 0;
    return b;
}

struct EncBufs { void* a_patch; BlockBufs blk; size_t bytes; };
EncBufs carve_encoder(const bd_dino_weights* w, int n, int prec, void* ws) {
    Carver c{(unsigned char*)ws, 0};
    const int np = planes_of(prec), P = w->grid * w->grid;
    EncBufs e;
    e.a_patch = c.take((size_t)n * P * w->kpad * 2 * np);
    e.blk = carve_block(c, (int64_t)n * (P + w->n_prefix), w->dim, np, w->latency_mode != 0);
    e.bytes = c.off + 256;
    return e;
}

// The decoder's one workspace layout, in take() order: a_heat, t1, t2, rgb, qtok, proj, blk.  What a call lacks takes no bytes and does
// not move the offset:
//   heat   the heat-map patch operand, and the adapter's buffers (t1, t2, rgb) on all n_views * P rows (the heat-map entry of
//          decoder_chain, bd_decoder_entry_tokens); without it the adapter runs on the B * P query rows (the banked entry)
//   stack  the head's buffers (qtok, proj) and the block buffers on all n_views * P rows (every forward; not bd_decoder_entry_tokens)
// n_views: views of the whole batch (B * T, or the sum of a ragged batch's view counts): every buffer is sized by token rows, none by T
struct DecBufs { void *a_heat, *t1, *qtok; float *t2, *rgb, *proj; BlockBufs blk; size_t bytes; };
DecBufs carve_decoder(const bd_betr_weights* w, int64_t n_views, int B, int prec, void* ws, bool heat, bool stack) {
    Carver c{(unsigned char*)ws, 0};
    const int np = planes_of(prec), P = w->grid * w->grid, D = w->dim;
    const int64_t Mb = n_views * P, Mq = (int64_t)B * P, Ma = heat ? Mb : Mq;
    const int F = w->patch * w->patch * w->box_dim;
    DecBufs d{};
    if (heat) d.a_heat = c.take((size_t)Mb * w->kpad * 2 * np);
    d.t1 = c.take((size_t)Ma * D * 2 * np);
    d.t2 = (float*)c.take((size_t)Ma * D * 4);
    d.rgb = (float*)c.take((size_t)Ma * D * 4);
    if (stack) {
        d.qtok = c.take((size_t)Mq * D * 2 * np);
        d.proj = (float*)c.take((size_t)Mq * F * 4);
        d.blk = carve_block(c, Mb, D, np, w->latency_mode != 0);
    }
    d.bytes = c.off + 256;
    return d;
}

inline bool bad_prec(int prec) {
    return prec != BD_PREC_BF16 && prec != BD_PREC_F16 && prec != BD_PREC_BF16X3 && prec != BD_PREC_FP8 &&
           prec != BD_PREC_BF16X3_ATTN_X3 && prec != BD_PREC_F16C8 && prec != BD_PREC_F16C8_QK16 && prec != BD_PREC_F16X3 &&
           prec != BD_PREC_F16X3_ATTN_X3;
}

}  // namespace

extern "C" int bd_abi_version(void) { return BD_ABI_VERSION; }
extern "C" const char* bd_target_arch(void) { return "gfx950"; }

extern "C" size_t bd_encoder_workspace_bytes(const bd_dino_weights* w, int n_images, int prec) {
    if (!w || n_images <= 0 || bad_prec(prec)) return 0;
    return carve_encoder(w, n_images, prec, nullptr).bytes;
}

extern "C" int bd_encoder_forward(const bd_dino_weights* w, const void* images, int img_dtype, int n_images,
                                  int size, float* feats32, void* feats16, int64_t feats16_plane, void* workspace,
                                  size_t workspace_bytes, int wprec, void* stream) {
    if (!w || !images || !workspace || !w->blocks || (!feats32 && !feats16)) return BD_ERR_NULL;
    if (bad_prec(wprec)) return BD_ERR_DTYPE;
    const int prec = gemm_prec(wprec);      // operand class of the unit operators; wprec also carries the attention policy
    if (n_images <= 0 || size != w->grid * w->patch || w->dim % w->heads || w->kpad % 64 ||
        w->kpad < 3 * w->patch * w->patch)
        return BD_ERR_SHAPE;
    if (w->feats_prec != 0 && !(w->feats_prec == prec || w->feats_prec == promoted_class(prec))) return BD_ERR_DTYPE;
    const int feats_prec = w->feats_prec ? w->feats_prec : prec;
    if ((uintptr_t)workspace & 255) return BD_ERR_ALIGN;
    const EncBufs e = carve_encoder(w, n_images, prec, workspace);
    if (workspace_bytes < e.bytes) return BD_ERR_WORKSPACE;
    const int P = w->grid * w->grid, D = w->dim, tpi = P + w->n_prefix;
    const int Mp = n_images * P;
    Stack s{};
    s.blocks = w->blocks; s.depth = w->depth; s.b = e.blk;
    s.M = n_images * tpi; s.batch = n_images; s.seq = tpi; s.D = D; s.heads = w->heads; s.ln_eps = w->ln_eps; s.n_prefix = w->n_prefix;
    std::vector<BlockPlan> sched;
    BD_TRY(plan_stack(s, wprec, sched));
    if (e.blk.sk && hipMemsetAsync(e.blk.sk, 0, e.blk.sk_flag_bytes, (hipStream_t)stream) != hipSuccess) return BD_ERR_WORKSPACE;

    // K1+K2: normalise + im2col, then the patch-embed GEMM scattering rows b*P+p -> b*tpi+n_prefix+p and
    // adding the (pre-resampled) positional table  (vision_transformer.py:213-232, patch_embed.py:65-75)
    const int c_pe = lin_class(prec, (prec == BD_PREC_F16C8 || prec == BD_PREC_FP8) ? w->promote_misc : 0, BD_PROMOTE_PATCH_EMBED);
    BD_TRY(bd_im2col_images(images, img_dtype, e.a_patch, (int64_t)Mp * w->kpad, n_images, size, w->patch, w->kpad,
                            c_pe, stream));
    {
        bd_gemm_args g = gemm_args(e.a_patch, w->kpad, (int64_t)Mp * w->kpad, w->patch_embed, w->kpad, D, e.blk.x, D, 0,
                                   1, Mp, w->kpad, BD_ACT_NONE);
        g.addtab = w->pos_patch; g.tab_rows = P;
        g.rpg_in = P; g.rpg_out = tpi; g.row_off = w->n_prefix;
        BD_TRY(bd_gemm(&g, c_pe, stream));
    }
    BD_TRY(bd_write_prefix_tokens(e.blk.x, w->prefix_tokens, n_images, tpi, w->n_prefix, D, stream));
    for (const BlockPlan& b : sched) BD_TRY(run_block(b, s, stream));
    // final LayerNorm on the patch tokens only (vision_transformer.py:263-267); feats16 in the class the consumer's first Linear reads
    BD_TRY(bd_layernorm(e.blk.x, D, w->norm_w, w->norm_b, w->ln_eps, feats16, feats16_plane, feats32, D, Mp, D, P, tpi,
                        w->n_prefix, feats_prec, stream));
    return BD_OK;
}

extern "C" size_t bd_decoder_workspace_bytes(const bd_betr_weights* w, int B, int T, int prec) {
    if (!w || B <= 0 || T <= 0 || bad_prec(prec)) return 0;
    return carve_decoder(w, (int64_t)B * T, B, prec, nullptr, true, true).bytes;
}

namespace {

// operand classes of the Linears outside the blocks (F16C8 family: per-Linear promotion, include/boxdreamer_hip.h)
struct MiscClasses { int a1, a2, be, bp; };
inline MiscClasses misc_classes(const bd_betr_weights* w, int prec) {
    const int pm0 = (prec == BD_PREC_F16C8 || prec == BD_PREC_FP8) ? w->promote_misc : 0;
    const int pmisc = (pm0 & BD_PROMOTE_ADAPTER_FC1) ? (pm0 | BD_PROMOTE_ADAPTER_FC2) : pm0;
    return {lin_class(prec, pmisc, BD_PROMOTE_ADAPTER_FC1), lin_class(prec, pmisc, BD_PROMOTE_ADAPTER_FC2),
            lin_class(prec, pmisc, BD_PROMOTE_BBOX_EMB), lin_class(prec, pmisc, BD_PROMOTE_BBOX_PROJ)};
}

// K6 adapter on M rows: rgb = LN_noaffine(fc2(gelu(fc1(feat))))  (betr.py:313-317); feats16 arrives in the class of adapter fc1
int adapter_rows(const bd_betr_weights* w, const MiscClasses& c, const void* feats16, int64_t feats16_plane, int M, void* t1, float* t2,
                 float* rgb, int prec, void* stream) {
    const int D = w->dim;
    const int64_t pD = (int64_t)M * D;
    {
        bd_gemm_args g = gemm_args(feats16, D, feats16_plane, w->adapter_fc1, D, D, t1, D, pD, handoff_kind(c.a1, c.a2), M, D, BD_ACT_GELU);
        BD_TRY(bd_gemm(&g, c.a1, stream));
    }
    {
        bd_gemm_args g = gemm_args(t1, D, pD, w->adapter_fc2, D, D, t2, D, 0, 1, M, D, BD_ACT_NONE);
        BD_TRY(bd_gemm(&g, c.a2, stream));
    }
    return bd_layernorm(t2, D, nullptr, nullptr, w->adapter_ln_eps, nullptr, 0, rgb, D, M, D, 0, 0, 0, prec, stream);
}

// K7+K8 on n_views views: x = bbox_emb(patchify(bbox_feat)) + rgb + pos, the heat-map patch embedding fused with its two additions
// (betr.py:324-329, 367-399)
int entry_rows(const bd_betr_weights* w, const MiscClasses& c, const void* bbox_feat, int in_dtype, int n_views, int size, void* a_heat,
               const float* rgb, float* x, void* stream) {
    const int P = w->grid * w->grid, D = w->dim, M = n_views * P;
    BD_TRY(bd_patchify_heatmaps(bbox_feat, in_dtype, a_heat, (int64_t)M * w->kpad, n_views, w->box_dim, size, w->patch, w->kpad, c.be, stream));
    bd_gemm_args g = gemm_args(a_heat, w->kpad, (int64_t)M * w->kpad, w->bbox_emb, w->kpad, D, x, D, 0, 1, M, w->kpad, BD_ACT_NONE);
    g.addtab = w->pos_table; g.tab_rows = P;
    g.resid = rgb; g.ldr = D;
    return bd_gemm(&g, c.be, stream);
}

// Where a call's decoder-entry tokens come from; exactly one of the two sources is set.
//   heat maps (bank == false): bbox_feat in in_dtype, one map per view; feats16 then covers all n_views views
//   a bank    (bank == true):  banked entry rows bank_x [bank_views, P, D] and the views' source table src (include/boxdreamer_hip.h,
//                              bd_assemble_entry_tokens_from); feats16 then covers the B query views.  `first`: a sub-batch lane's samples
//                              are [first, first + B) of the batch, and src names their queries by the batch's numbering
struct EntrySource {
    bool bank;
    const void* bbox_feat; int in_dtype;
    const float* bank_x; int bank_views; const int32_t* src; int first;
};
inline EntrySource heat_source(const void* bbox_feat, int in_dtype) { return {false, bbox_feat, in_dtype, nullptr, 0, nullptr, 0}; }
inline EntrySource bank_source(const float* bank_x, int bank_views, const int32_t* src, int first) {
    return {true, nullptr, 0, bank_x, bank_views, src, first};
}

inline bool bad_betr_shape(const bd_betr_weights* w, int size) {
    return size != w->grid * w->patch || w->dim % w->heads || w->kpad % 64 || w->box_dim != 8 || w->kpad < w->patch * w->patch * w->box_dim;
}

// The argument checks of every decoder entry point, in one order; nothing is dereferenced but w, nothing enqueued.  `stack`: the call runs
// the block stack and the head (a forward; bd_decoder_entry_tokens only builds rows: B = n_views free-standing views, T = 1).  `ragged`:
// the samples' views are given by view_start, T is the largest per-sample count.  `out`: any one of the call's outputs.
int check_decoder_call(const bd_betr_weights* w, const EntrySource& e, const void* feats16, const int32_t* view_start, const int32_t* query_idx,
                       bool ragged, bool stack, int B, int64_t n_views, int T, int size, const void* out, const void* workspace, int wprec) {
    if (!w || !feats16 || !out || !workspace) return BD_ERR_NULL;
    if (e.bank ? (!e.src || (e.bank_views > 0 && !e.bank_x)) : !e.bbox_feat) return BD_ERR_NULL;
    if (stack && (!query_idx || !w->blocks || (ragged && !view_start))) return BD_ERR_NULL;
    if (bad_prec(wprec)) return BD_ERR_DTYPE;
    if (!e.bank && (e.in_dtype < 0 || e.in_dtype > 2)) return BD_ERR_DTYPE;
    if (B <= 0 || T <= 0 || n_views < B || (e.bank && e.bank_views < 0) || bad_betr_shape(w, size)) return BD_ERR_SHAPE;
    if (ragged) {
        if (T > n_views - (B - 1) || (int64_t)T * B < n_views) return BD_ERR_SHAPE;       // no set of B view counts has this sum and maximum
        if ((w->grid * w->grid) % 128 || w->dim / w->heads != 96) return BD_ERR_SHAPE;      // what bd_attention_varlen takes
    }
    if (n_views * w->grid * w->grid >= ((int64_t)1 << 31)) return BD_ERR_SHAPE;             // token rows are counted in int
    if ((uintptr_t)workspace & 255) return BD_ERR_ALIGN;
    return BD_OK;
}

// The decoder chain on n_views * P packed token rows, for every forward.  Entry tokens by their source: from heat maps, the adapter runs on
// all rows, the heat-map embedding adds rgb + pos and the query rows are substituted; from a bank, the adapter runs on the B * P query rows
// and one launch assembles the stream from the banked rows and the query rows -- then the same Stack, the same plan, the same head.
// !ragged: a uniform batch (n_views = B * T, every sample T views).  ragged: the same launches; attention, the query-token substitution and
// the query-row gather take the sample boundaries from view_start, everything else is row-wise and sees M = n_views * P.
int decoder_chain(const bd_betr_weights* w, const EntrySource& e, const void* feats16, int64_t feats16_plane, const int32_t* view_start,
                  const int32_t* query_idx, bool ragged, int B, int64_t views, int T, int size, float* logits, float* heat, void* workspace,
                  size_t workspace_bytes, int wprec, void* stream) {
    BD_TRY(check_decoder_call(w, e, feats16, view_start, query_idx, ragged, true, B, views, T, size, logits ? logits : heat, workspace, wprec));
    const int prec = gemm_prec(wprec), n_views = (int)views;
    const DecBufs d = carve_decoder(w, n_views, B, prec, workspace, !e.bank, true);
    if (workspace_bytes < d.bytes) return BD_ERR_WORKSPACE;
    const int P = w->grid * w->grid, D = w->dim, F = w->patch * w->patch * w->box_dim;
    const int Mb = n_views * P, Mq = B * P;
    // K9: joint self-attention over all T*P tokens of a sample; the last block runs the query view's rows only past K / V, on d.t2 (dead
    // since the adapter) as its compact stream
    Stack s{};
    s.blocks = w->blocks; s.depth = w->depth; s.b = d.blk;
    s.M = Mb; s.batch = B; s.seq = T * P; s.D = D; s.heads = w->heads; s.ln_eps = w->ln_eps; s.rms_eps = w->rms_eps;
    s.lat = !ragged && w->latency_mode && Mb <= BD_SPLITK_MAX_ROWS; s.query_idx = query_idx; s.P = P; s.xc = d.t2;
    s.view_start = ragged ? view_start : nullptr; s.n_views = n_views; s.max_views = T;      // (ragged: T is the largest per-sample view count)
    std::vector<BlockPlan> sched;
    BD_TRY(plan_stack(s, wprec, sched));
    if (d.blk.sk && hipMemsetAsync(d.blk.sk, 0, d.blk.sk_flag_bytes, (hipStream_t)stream) != hipSuccess) return BD_ERR_WORKSPACE;

    const MiscClasses c = misc_classes(w, prec);
    if (e.bank) {
        // K6 on the query views only, then the stream: banked rows as they are, the query rows (query_token + rgb) + pos  (betr.py:286-290)
        BD_TRY(adapter_rows(w, c, feats16, feats16_plane, Mq, d.t1, d.t2, d.rgb, prec, stream));
        BD_TRY(bd_assemble_entry_tokens_from(e.bank_x, e.bank_views, d.rgb, e.first, B, w->pos_table, w->query_token, e.src, d.blk.x, n_views, P,
                                             D, stream));
    } else {
        BD_TRY(adapter_rows(w, c, feats16, feats16_plane, Mb, d.t1, d.t2, d.rgb, prec, stream));
        BD_TRY(entry_rows(w, c, e.bbox_feat, e.in_dtype, n_views, size, d.a_heat, d.rgb, d.blk.x, stream));
        if (ragged) BD_TRY(bd_query_substitute_varlen(d.blk.x, d.rgb, w->pos_table, w->query_token, view_start, query_idx, B, P, D, stream));
        else BD_TRY(bd_query_substitute(d.blk.x, d.rgb, w->pos_table, w->query_token, query_idx, B, T, P, D, stream));
    }
    for (const BlockPlan& b : sched) BD_TRY(run_block(b, s, stream));
    // K10: head on the query view's tokens (no final norm, betr.py:298-306)
    BD_TRY(bd_gather_query_tokens(d.t2, nullptr, d.qtok, (int64_t)Mq * D, B, 1, P, D, c.bp, stream));
    {
        bd_gemm_args g = gemm_args(d.qtok, D, (int64_t)Mq * D, w->bbox_proj, D, F, d.proj, F, 0, 1, Mq, D, BD_ACT_NONE);
        BD_TRY(bd_gemm(&g, c.bp, stream));
    }
    return bd_unpatchify_sigmoid(d.proj, logits, heat, B, w->box_dim, size, w->patch, stream);
}
}  // namespace

extern "C" int bd_decoder_forward(const bd_betr_weights* w, const void* bbox_feat, int in_dtype, const void* feats16,
                                  int64_t feats16_plane, const int32_t* query_idx, int B, int T, int size,
                                  float* logits, float* heat, void* workspace, size_t workspace_bytes, int wprec,
                                  void* stream) {
    return decoder_chain(w, heat_source(bbox_feat, in_dtype), feats16, feats16_plane, nullptr, query_idx, false, B, (int64_t)B * T, T, size,
                         logits, heat, workspace, workspace_bytes, wprec, stream);
}

extern "C" size_t bd_decoder_workspace_bytes_ragged(const bd_betr_weights* w, int n_views, int B, int prec) {
    if (!w || B <= 0 || n_views < B || bad_prec(prec)) return 0;
    return carve_decoder(w, n_views, B, prec, nullptr, true, true).bytes;
}

extern "C" int bd_decoder_forward_ragged(const bd_betr_weights* w, const void* bbox_feat, int in_dtype, const void* feats16,
                                         int64_t feats16_plane, const int32_t* view_start, const int32_t* query_view, int B, int n_views,
                                         int max_views, int size, float* logits, float* heat, void* workspace, size_t workspace_bytes,
                                         int wprec, void* stream) {
    return decoder_chain(w, heat_source(bbox_feat, in_dtype), feats16, feats16_plane, view_start, query_view, true, B, n_views, max_views,
                         size, logits, heat, workspace, workspace_bytes, wprec, stream);
}

// ----------------------------------------------------------------------------------------------------------------------------
// Sub-batch lanes.  Samples are independent all the way down the path, and every row's result is independent
// of the tile shape its launch picks (tests/test_gpu_ops.py::test_gemm_row_result_independent_of_tile_shape, the batch-invariance
// tests), so ONE batch may run as `lanes` contiguous sub-batches on `lanes` streams without changing a bit of the result: lane 0 on
// the caller's stream, the others on side streams this library owns, forked from and joined back into the caller's stream with
// events inside the call -- the call stays stream-ordered for the caller (and capturable: an event wait pulls the side stream into
// the caller's capture).  What it buys: the kernels of one lane run on the CUs the other lane's ragged last round leaves idle and
// the HBM-bound launches (LayerNorm) of one lane overlap the MFMA-bound launches of the other -- what two BATCHES in flight bought
// in rounds 2-4, now inside one batch of configs[1] (profiles/r4_subbatch_lanes.md).
namespace {

constexpr int kMaxLanes = 4, kMaxDevices = 64;
struct LaneSet {
    hipStream_t side[kMaxLanes - 1];
    hipEvent_t fork, join[kMaxLanes - 1];
    bool ready = false;
};
// Per HOST THREAD and device (round 6; process-global until then): a thread that captures `stream` into a HIP graph pulls ITS OWN side
// streams into the capture and nobody else's -- two threads may enqueue laned calls on one device at the same time, capturing or not.
// Created on first use (or by bd_lanes_prepare), never destroyed: a thread that exits leaves its three streams / four events behind.
thread_local LaneSet g_lanes[kMaxDevices];

int lanes_of_current_device(LaneSet** out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev < 0 || dev >= kMaxDevices) return BD_ERR_SHAPE;
    LaneSet& L = g_lanes[dev];
    if (!L.ready) {
        if ((e = hipEventCreateWithFlags(&L.fork, hipEventDisableTiming)) != hipSuccess) return (int)e;
        for (int i = 0; i < kMaxLanes - 1; ++i) {
            if ((e = hipStreamCreateWithFlags(&L.side[i], hipStreamNonBlocking)) != hipSuccess) return (int)e;
            if ((e = hipEventCreateWithFlags(&L.join[i], hipEventDisableTiming)) != hipSuccess) return (int)e;
        }
        L.ready = true;
    }
    *out = &L;
    return BD_OK;
}

inline int lane_count(int lanes, int units) { return lanes < 1 ? 1 : (lanes > kMaxLanes ? kMaxLanes : (lanes > units ? units : lanes)); }
inline int lane_units(int units, int lanes, int l) { return units / lanes + (l < units % lanes ? 1 : 0); }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Lane l of nl: its units [first, first + count) of the batch and its slice [woff, woff + bytes) of the workspace.  bytes_of(count) is
// the aligned carve size of a lane of `count` units: the laned forwards and the *_workspace_bytes*_lanes totals split with the same one.
struct LaneSlice { int first, count; size_t woff, bytes; };
template <class F> LaneSlice lane_slice(int units, int nl, int l, const F& bytes_of) {
    LaneSlice s{0, lane_units(units, nl, l), 0, 0};
    for (int j = 0; j < l; ++j) {
        s.first += lane_units(units, nl, j);
        s.woff += bytes_of(lane_units(units, nl, j));
    }
    s.bytes = bytes_of(s.count);
    return s;
}
template <class F> size_t lanes_total(int units, int nl, const F& bytes_of) {
    const LaneSlice last = lane_slice(units, nl, nl - 1, bytes_of);
    return last.woff + last.bytes;
}
inline auto encoder_lane_bytes(const bd_dino_weights* w, int prec) {
    return [=](int n) { return align256(carve_encoder(w, n, gemm_prec(prec), nullptr).bytes); };
}
// (a lane of b samples at T views each; heat: the heat-map entry's layout, else the banked entry's -- carve_decoder)
inline auto decoder_lane_bytes(const bd_betr_weights* w, int T, int prec, bool heat) {
    return [=](int b) { return align256(carve_decoder(w, (int64_t)b * T, b, gemm_prec(prec), nullptr, heat, true).bytes); };
}

// element offset e0 into a 16-bit operand buffer of class `cls`: plane 0 moves by e0 elements; F16C8's one-byte lo8 plane (which
// starts `plane` 2-byte units behind plane 0) moves by e0 BYTES, i.e. the plane distance seen from the moved base shrinks by e0 / 2
inline void operand_slice(const void* base, int64_t plane, int cls, int64_t e0, const void** b, int64_t* p) {
    const int esz = cls == BD_PREC_FP8 ? 1 : 2;
    *b = base ? (const unsigned char*)base + e0 * esz : nullptr;
    *p = cls == BD_PREC_F16C8 ? plane - e0 / 2 : plane;
}
inline int dtype_bytes(int dt) { return dt == BD_DTYPE_F32 ? 4 : 2; }

// fork / join around the per-lane calls.  Every lane is enqueued even after an earlier one failed, and the joins are always
// recorded, so that a capture in progress is left well-formed; the first error is returned.
template <class F> int run_lanes(int lanes, hipStream_t main, F&& lane_call) {
    LaneSet* L = nullptr;
    BD_TRY(lanes_of_current_device(&L));
    hipError_t e = hipEventRecord(L->fork, main);
    if (e != hipSuccess) return (int)e;
    int rc = BD_OK;
    bd_concurrent_launches() = lanes;          // the lanes' launches run side by side: tile-form choices count a lane's share of the CUs
    for (int l = 0; l < lanes; ++l) {
        hipStream_t s = l == 0 ? main : L->side[l - 1];
        if (l > 0 && (e = hipStreamWaitEvent(s, L->fork, 0)) != hipSuccess && rc == BD_OK) rc = (int)e;
        const int r = lane_call(l, s);
        if (r != BD_OK && rc == BD_OK) rc = r;
    }
    bd_concurrent_launches() = 1;
    for (int l = 1; l < lanes; ++l) {
        if ((e = hipEventRecord(L->join[l - 1], L->side[l - 1])) != hipSuccess && rc == BD_OK) rc = (int)e;
        if ((e = hipStreamWaitEvent(main, L->join[l - 1], 0)) != hipSuccess && rc == BD_OK) rc = (int)e;
    }
    return rc;
}

}  // namespace

extern "C" int bd_lanes_prepare(void) {
    LaneSet* L = nullptr;
    return lanes_of_current_device(&L);
}

extern "C" size_t bd_encoder_workspace_bytes_lanes(const bd_dino_weights* w, int n_images, int prec, int lanes) {
    if (!w || n_images <= 0 || bad_prec(prec)) return 0;
    return lanes_total(n_images, lane_count(lanes, n_images), encoder_lane_bytes(w, prec));
}

extern "C" int bd_encoder_forward_lanes(const bd_dino_weights* w, const void* images, int img_dtype, int n_images, int size,
                                        float* feats32, void* feats16, int64_t feats16_plane, void* workspace,
                                        size_t workspace_bytes, int wprec, int lanes, void* stream) {
    const int nl = lane_count(lanes, n_images);
    if (nl <= 1 || !w) return bd_encoder_forward(w, images, img_dtype, n_images, size, feats32, feats16, feats16_plane, workspace,
                                                 workspace_bytes, wprec, stream);
    if (bad_prec(wprec)) return BD_ERR_DTYPE;
    if (!images || !workspace) return BD_ERR_NULL;
    if (img_dtype < 0 || img_dtype > 2) return BD_ERR_DTYPE;
    if ((uintptr_t)workspace & 255) return BD_ERR_ALIGN;
    const auto lane_bytes = encoder_lane_bytes(w, wprec);
    if (workspace_bytes < lanes_total(n_images, nl, lane_bytes)) return BD_ERR_WORKSPACE;
    const int fcls = w->feats_prec ? w->feats_prec : gemm_prec(wprec);
    const int64_t PD = (int64_t)w->grid * w->grid * w->dim, img_elems = (int64_t)3 * size * size;
    return run_lanes(nl, (hipStream_t)stream, [&](int l, hipStream_t s) {
        const LaneSlice ln = lane_slice(n_images, nl, l, lane_bytes);
        const void* f16 = nullptr;
        int64_t plane = feats16_plane;
        operand_slice(feats16, feats16_plane, fcls, ln.first * PD, &f16, &plane);
        return bd_encoder_forward(w, (const unsigned char*)images + ln.first * img_elems * dtype_bytes(img_dtype), img_dtype, ln.count, size,
                                  feats32 ? feats32 + ln.first * PD : nullptr, const_cast<void*>(f16), plane,
                                  (unsigned char*)workspace + ln.woff, ln.bytes, wprec, s);
    });
}

extern "C" size_t bd_decoder_workspace_bytes_lanes(const bd_betr_weights* w, int B, int T, int prec, int lanes) {
    if (!w || B <= 0 || T <= 0 || bad_prec(prec)) return 0;
    return lanes_total(B, lane_count(lanes, B), decoder_lane_bytes(w, T, prec, true));
}

extern "C" int bd_decoder_forward_lanes(const bd_betr_weights* w, const void* bbox_feat, int in_dtype, const void* feats16,
                                        int64_t feats16_plane, const int32_t* query_idx, int B, int T, int size, float* logits,
                                        float* heat, void* workspace, size_t workspace_bytes, int wprec, int lanes, void* stream) {
    const int nl = lane_count(lanes, B);
    if (nl <= 1 || !w) return bd_decoder_forward(w, bbox_feat, in_dtype, feats16, feats16_plane, query_idx, B, T, size, logits, heat,
                                                 workspace, workspace_bytes, wprec, stream);
    // (the whole batch's arguments and the laned workspace total are checked before the fork: a bad call records no event)
    BD_TRY(check_decoder_call(w, heat_source(bbox_feat, in_dtype), feats16, nullptr, query_idx, false, true, B, (int64_t)B * T, T, size,
                              logits ? logits : heat, workspace, wprec));
    const auto lane_bytes = decoder_lane_bytes(w, T, wprec, true);
    if (workspace_bytes < lanes_total(B, nl, lane_bytes)) return BD_ERR_WORKSPACE;
    const int fcls = misc_classes(w, gemm_prec(wprec)).a1;       // the class bd_decoder_forward reads feats16 in
    const int64_t PD = (int64_t)w->grid * w->grid * w->dim, view_elems = (int64_t)w->box_dim * size * size;
    return run_lanes(nl, (hipStream_t)stream, [&](int l, hipStream_t s) {
        const LaneSlice ln = lane_slice(B, nl, l, lane_bytes);
        const int64_t v0 = (int64_t)ln.first * T;                  // the lane's first view
        const void* f16 = nullptr;
        int64_t plane = feats16_plane;
        operand_slice(feats16, feats16_plane, fcls, v0 * PD, &f16, &plane);
        return bd_decoder_forward(w, (const unsigned char*)bbox_feat + v0 * view_elems * dtype_bytes(in_dtype), in_dtype, f16, plane,
                                  query_idx + ln.first, ln.count, T, size, logits ? logits + ln.first * view_elems : nullptr,
                                  heat ? heat + ln.first * view_elems : nullptr, (unsigned char*)workspace + ln.woff, ln.bytes, wprec, s);
    });
}

// ----------------------------------------------------------------------------------------------------------------------------
// Decoder-entry tokens kept in a bank (include/boxdreamer_hip.h).  A reference's entry row -- bbox_emb(patchify(bbox_feat)) + pos +
// adapter(feat), betr.py:313-329 and :367-399 -- is row-wise and independent of the query: bd_decoder_entry_tokens computes it once,
// with the heat-map entry's own five launches (adapter_rows, entry_rows), and bd_decoder_forward_entry[_ragged] is decoder_chain with the
// bank as its entry source: the adapter on the query rows alone, one launch that assembles the token stream from the banked rows, then
// the one block stack and head.

extern "C" size_t bd_decoder_entry_tokens_workspace_bytes(const bd_betr_weights* w, int n_views, int prec) {
    if (!w || n_views <= 0 || bad_prec(prec)) return 0;
    return carve_decoder(w, n_views, 0, gemm_prec(prec), nullptr, true, false).bytes;
}

extern "C" int bd_decoder_entry_tokens(const bd_betr_weights* w, const void* bbox_feat, int in_dtype, const void* feats16,
                                       int64_t feats16_plane, int n_views, int size, float* x_out, void* workspace,
                                       size_t workspace_bytes, int wprec, void* stream) {
    // (n_views free-standing views: each its own sample of one view)
    BD_TRY(check_decoder_call(w, heat_source(bbox_feat, in_dtype), feats16, nullptr, nullptr, false, false, n_views, n_views, 1, size, x_out,
                              workspace, wprec));
    const int prec = gemm_prec(wprec);
    const DecBufs t = carve_decoder(w, n_views, 0, prec, workspace, true, false);
    if (workspace_bytes < t.bytes) return BD_ERR_WORKSPACE;
    const MiscClasses c = misc_classes(w, prec);
    BD_TRY(adapter_rows(w, c, feats16, feats16_plane, n_views * w->grid * w->grid, t.t1, t.t2, t.rgb, prec, stream));
    return entry_rows(w, c, bbox_feat, in_dtype, n_views, size, t.a_heat, t.rgb, x_out, stream);
}

extern "C" size_t bd_decoder_entry_workspace_bytes_ragged(const bd_betr_weights* w, int n_views, int B, int prec) {
    if (!w || B <= 0 || n_views < B || bad_prec(prec)) return 0;
    return carve_decoder(w, n_views, B, gemm_prec(prec), nullptr, false, true).bytes;
}

extern "C" size_t bd_decoder_entry_workspace_bytes(const bd_betr_weights* w, int B, int T, int prec, int lanes) {
    if (!w || B <= 0 || T <= 0 || bad_prec(prec)) return 0;
    return lanes_total(B, lane_count(lanes, B), decoder_lane_bytes(w, T, prec, false));
}

extern "C" int bd_decoder_forward_entry(const bd_betr_weights* w, const float* bank_x, int bank_views, const int32_t* src,
                                        const void* feats16, int64_t feats16_plane, const int32_t* query_idx, int B, int T, int size,
                                        float* logits, float* heat, void* workspace, size_t workspace_bytes, int wprec, int lanes,
                                        void* stream) {
    const int nl = lane_count(lanes, B);
    const int64_t n_views = (int64_t)B * T;
    if (nl <= 1 || !w) return decoder_chain(w, bank_source(bank_x, bank_views, src, 0), feats16, feats16_plane, nullptr, query_idx, false, B,
                                            n_views, T, size, logits, heat, workspace, workspace_bytes, wprec, stream);
    // (the whole batch's arguments and the laned workspace total are checked before the fork: a bad call records no event)
    BD_TRY(check_decoder_call(w, bank_source(bank_x, bank_views, src, 0), feats16, nullptr, query_idx, false, true, B, n_views, T, size,
                              logits ? logits : heat, workspace, wprec));
    const auto lane_bytes = decoder_lane_bytes(w, T, wprec, false);
    if (workspace_bytes < lanes_total(B, nl, lane_bytes)) return BD_ERR_WORKSPACE;
    const int fcls = misc_classes(w, gemm_prec(wprec)).a1;       // the class the adapter's first Linear reads feats16 in
    const int64_t PD = (int64_t)w->grid * w->grid * w->dim, map_elems = (int64_t)w->box_dim * size * size;
    return run_lanes(nl, (hipStream_t)stream, [&](int l, hipStream_t s) {
        const LaneSlice ln = lane_slice(B, nl, l, lane_bytes);
        const void* f16 = nullptr;
        int64_t plane = feats16_plane;
        operand_slice(feats16, feats16_plane, fcls, ln.first * PD, &f16, &plane);     // (one query view per sample)
        return decoder_chain(w, bank_source(bank_x, bank_views, src + (int64_t)ln.first * T, ln.first), f16, plane, nullptr,
                             query_idx + ln.first, false, ln.count, (int64_t)ln.count * T, T, size,
                             logits ? logits + ln.first * map_elems : nullptr, heat ? heat + ln.first * map_elems : nullptr,
                             (unsigned char*)workspace + ln.woff, ln.bytes, wprec, s);
    });
}

extern "C" int bd_decoder_forward_entry_ragged(const bd_betr_weights* w, const float* bank_x, int bank_views, const int32_t* src,
                                               const void* feats16, int64_t feats16_plane, const int32_t* view_start,
                                               const int32_t* query_view, int B, int n_views, int max_views, int size, float* logits,
                                               float* heat, void* workspace, size_t workspace_bytes, int wprec, void* stream) {
    return decoder_chain(w, bank_source(bank_x, bank_views, src, 0), feats16, feats16_plane, view_start, query_view, true, B, n_views,
                         max_views, size, logits, heat, workspace, workspace_bytes, wprec, stream);
}
