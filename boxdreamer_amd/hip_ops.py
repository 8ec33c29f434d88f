"""Thin tensor-level wrappers over the C ABI (one function per exported operator).

Used by the GPU parity tests and by the module mirrors.  All tensors must live on the HIP device;
every call is enqueued on torch's current stream.  In the "bf16x3" mode a 16-bit activation is a
stacked pair [2, rows, cols] (hi plane, lo plane).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, operand
from ._lib import check, planes, prec_id, ptr, stream

E4M3_MAX = 448.0


def f16c8_qexp(w: torch.Tensor) -> int:
    """Exponent E of a weight tensor's e4m3 planes: the largest power of two that keeps max|w| * 2^E inside e4m3."""
    m = float(w.detach().abs().max())
    return 0 if m <= 0 else int(torch.floor(torch.log2(torch.tensor(E4M3_MAX / m))).item())


def _f16c8_perm(K: int, device) -> torch.Tensor:
    """Byte position -> k inside every 32-block of the lo8 plane: byte 16 h + 8 a + j holds k = 16 a + 8 h + j."""
    pos = torch.arange(32, device=device)
    h, a, j = pos // 16, (pos // 8) % 2, pos % 8
    k_of_pos = 16 * a + 8 * h + j
    return (torch.arange(0, K, 32, device=device)[:, None] + k_of_pos[None, :]).reshape(-1)


def f16c8_encode(x: torch.Tensor, qexp: int = 0, weight: bool = False) -> torch.Tensor:
    """fp32 [rows, K] (K % 32 == 0) -> [2, rows, K] float16 STORAGE of the F16C8 operand class (include/boxdreamer_hip.h):
    plane 0 = f16(x) (clamped to f16's finite range only); plane 1 = raw bytes (both e4m3 images saturate at +-448):
      activations: the first rows*K bytes are the lo8 plane e4m3((x - hi) 2^D), k-permuted per 32-block (rest unused);
      weights:     per 32-block 64 bytes = for each lane half h: [q8 x 16 | lo8 x 16] of its sixteen k (same k order),
                   q8 = e4m3(hi 2^E), lo8 = e4m3((w - hi) 2^(E + D)).
    The residual is taken against the fp32 value itself (csrc/bd_common.h: f16c8_split), so beyond +-65504 hi is the saturated f16 and
    lo8 the saturated image of what hi left over.
    Torch ops: weight packing at load time and test helpers (not on the hot path)."""
    x = x.float()
    rows, K = x.shape
    assert K % 32 == 0, "F16C8 operands are laid out in 32-element blocks"
    hi = x.clamp(-65504.0, 65504.0).half()
    lo = (x - hi.float()) * 2.0 ** (qexp + _lib.F16C8_D)
    perm = _f16c8_perm(K, x.device)
    l8 = lo.clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)[:, perm]
    if weight:
        q8 = (hi.float() * 2.0 ** qexp).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)[:, perm]
        mix = torch.stack([q8.reshape(rows, K // 16, 16), l8.reshape(rows, K // 16, 16)], dim=2)     # [rows, K/16, 2, 16]
        plane1 = mix.reshape(-1).contiguous()
    else:
        plane1 = torch.zeros((rows * K * 2,), dtype=torch.uint8, device=x.device)
        plane1[: rows * K] = l8.reshape(-1)
    return torch.stack([hi, plane1.view(torch.float16).reshape(rows, K)]).contiguous()


def f16c8_decode(t: torch.Tensor, qexp: int = 0, weight: bool = False):
    """(hi, lo, q) as fp32 [rows, K] -- exactly the three values the GEMM multiplies."""
    hi = t[0].float()
    rows, K = hi.shape
    raw = t[1].contiguous().view(torch.uint8).reshape(-1)
    inv = torch.empty(K, dtype=torch.long, device=t.device)
    inv[_f16c8_perm(K, t.device)] = torch.arange(K, device=t.device)
    dec = lambda b: b[:, inv].contiguous().view(torch.float8_e4m3fn).float()
    if weight:
        mix = raw.reshape(rows, K // 16, 2, 16)
        q = dec(mix[:, :, 0].reshape(rows, K)) * 2.0 ** -qexp
        lo = dec(mix[:, :, 1].reshape(rows, K)) * 2.0 ** -(qexp + _lib.F16C8_D)
    else:
        lo = dec(raw[: rows * K].reshape(rows, K)) * 2.0 ** -(qexp + _lib.F16C8_D)
        q = (hi * 2.0 ** qexp).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).float() * 2.0 ** -qexp     # derived by the GEMM in registers (saturating)
    return hi, lo, q


def to_operand(x: torch.Tensor, prec) -> torch.Tensor:
    """fp32 [rows, cols] -> operand tensor (test helper; torch ops, not on the product path)."""
    dt = _lib.op_dtype(prec)
    if prec_id(prec) == _lib.PREC_F16C8:
        return f16c8_encode(x, 0, False)
    if prec_id(prec) == _lib.PREC_FP8:
        return x.float().clamp(-448.0, 448.0).to(dt).contiguous()
    # the kernels' f16 conversions saturate (bd_common.h: RANGE), each on its own: lo is what the saturated hi left of the fp32 value
    sat = (lambda v: v.clamp(-65504.0, 65504.0)) if dt == torch.float16 else (lambda v: v)
    x = x.float()
    hi = sat(x).to(dt)
    if planes(prec) == 1:
        return hi.contiguous()
    return torch.stack([hi, sat(x - hi.float()).to(dt)]).contiguous()


def from_operand(t: torch.Tensor, prec) -> torch.Tensor:
    if prec_id(prec) == _lib.PREC_F16C8:
        hi, lo, _ = f16c8_decode(t)
        return hi + lo
    return t.float() if planes(prec) == 1 else t[0].float() + t[1].float()


_OUT_DTYPES = {2: torch.float16, 3: torch.bfloat16}      # single planes; 4 / 5: split-bf16 / split-f16 planes [2, rows, N]
_OUT_SPLIT = {4: torch.bfloat16, 5: torch.float16}


_FAMILY = {_lib.GEMM_FAMILY_PC: "pc", _lib.GEMM_FAMILY_GLDS: "glds", _lib.GEMM_FAMILY_PC_F16C8: "pc_f16c8"}


def gemm_plan(g, prec, cus=0, concurrent=1):
    """bd_gemm_plan (host only): the launches bd_gemm(g, prec) makes on a device of `cus` CUs (0: the current one), one dict each --
    family ("pc": persistent, "glds": one tile per workgroup, "pc_f16c8"), tile (rows, columns), stages (of the slab ring; "pc": 3 = the
    A3 / W2 operand ring, 2 = none), ep / outk / gelu / lnf (None for "glds": its epilogue is chosen at run time), split_k, grid, block,
    row0, rows, key.  Raises HipLibraryError where bd_gemm refuses the arguments."""
    plan = _lib.GemmPlan()
    check(_lib.load().bd_gemm_plan(C.byref(g), prec_id(prec), int(cus), int(concurrent), C.byref(plan)), "bd_gemm_plan")
    out = []
    for l in plan.launch[:plan.n_launches]:
        k = list(l.key)
        d = {"family": _FAMILY[l.family], "key": k, "grid": l.grid, "block": l.block, "row0": l.row0, "rows": l.rows, "split_k": l.split_k,
             "ep": None, "outk": None, "gelu": None, "lnf": None}
        if l.family == _lib.GEMM_FAMILY_PC_F16C8:
            d.update(tile=(k[4] * 64, k[5] * 96), stages=k[0], ep=k[1], outk=k[2], gelu=bool(k[3]), lnf=bool(k[7]))
        else:
            d.update(tile=(k[3] * k[5] * 32, k[4] * k[6] * 32))
            if l.family == _lib.GEMM_FAMILY_PC:
                d.update(stages=3 if k[11] else 2, ep=k[8], outk=k[9], gelu=bool(k[10]), lnf=bool(k[12]))
            else:
                d.update(stages=k[7])
        out.append(d)
    return out


def gemm_shape_args(M, N, K, **fields):
    """bd_gemm_args of an M x N x K launch on dense operands at made-up, aligned addresses: for asking gemm_plan about a shape before
    any tensor exists.  fields: further members, a pointer given as True (an aligned address)."""
    g = _lib.GemmArgs()
    g.M, g.N, g.K, g.lda, g.ldw, g.ldo, g.ldr, g.ln_op_ld = M, N, K, K, K, N, N, N
    g.a_plane = g.w_plane = g.out_plane = g.ln_op_plane = 1 << 28
    kinds = dict(_lib.GemmArgs._fields_)
    for i, name in enumerate(("A", "W", "out", "bias") + tuple(fields)):
        v = fields.get(name, True)
        setattr(g, name, (0x7F0000000000 + 0x1000 * (i + 1) if v else None) if kinds[name] is C.c_void_p and isinstance(v, bool) else v)
    return g


def _check_expect(g, prec, expect):
    """expect: what gemm_plan must say of the launch about to be made -- a dict (every launch has these values) or a list of dicts (one
    per launch, in order)."""
    plan = gemm_plan(g, prec)
    wants = expect if isinstance(expect, (list, tuple)) else [expect] * len(plan)
    assert len(wants) == len(plan), f"{len(plan)} launches planned, {len(wants)} expected: {plan}"
    for want, got in zip(wants, plan):
        for k, v in want.items():
            assert got[k] == (tuple(v) if k == "tile" else v), f"the plan's {k} is {got[k]}, the test expects {v}: {got}"


def gemm(a16, w16, bias=None, *, prec="bf16", act=_lib.ACT_NONE, resid=None, addtab=None, out=None,
         out_f32=False, n=None, out_rows=None, rpg=(0, 0, 0), wscale=None, out_mode=None, w_qexp=0, rms=None,
         ln_emit=None, ln_apply=None, ln_resid_in_op=False, split_k=None, expect=None):
    """out[map(r)] = act(wscale * (A W^T) + bias) + addtab[r % rows(addtab)] + resid[map(r)].
    out_mode: None -> operand dtype (or fp32 with out_f32), 2 -> f16 single plane, 3 -> bf16 single plane, 4 -> split-bf16 (hi, lo)
    planes, 5 -> split-f16 (hi, lo) planes (bd_gemm_args.out_f32, include/boxdreamer_hip.h).
    LayerNorm fold (ABI 8): ln_emit = (stats [M, N / 96, 2] fp32, operand copy [2, M, N] F16C8 storage) -- the producer side;
    ln_apply = (stats [M, 8, 2], column sums [N], eps) -- the consumer side.
    split_k = (scratch uint8 tensor of splitk_workspace_bytes(M, N) whose first 16 KiB are zero, factor 0 = library's choice | 2 .. 4):
    bd_gemm_args.sk_ws / sk_split (ABI 9).
    expect (tests): the kernel form this launch must take, checked against gemm_plan before the launch (_check_expect)."""
    lib = _lib.load()
    np_ = planes(prec)
    A2 = a16[0] if np_ == 2 else a16
    W2 = w16[0] if np_ == 2 else w16
    M, K = A2.shape
    N = n if n is not None else W2.shape[0]
    rows_out = out_rows if out_rows is not None else M
    mode = int(out_f32) if out_mode is None else out_mode
    if out is None:
        if mode == 1:
            out = torch.empty((rows_out, N), dtype=torch.float32, device=A2.device)
        elif mode in _OUT_DTYPES:
            out = torch.empty((rows_out, N), dtype=_OUT_DTYPES[mode], device=A2.device)
        elif mode in _OUT_SPLIT:
            out = torch.empty((2, rows_out, N), dtype=_OUT_SPLIT[mode], device=A2.device)
        else:
            out = operand.empty(prec, rows_out, N, A2.device)
    g = _lib.GemmArgs()
    g.A, g.lda, g.a_plane = ptr(a16), A2.stride(0), operand.plane_offset(a16, prec)
    g.W, g.ldw, g.w_plane = ptr(w16), W2.stride(0), operand.plane_offset(w16, prec)
    g.bias = ptr(bias)
    g.wscale = ptr(wscale)
    g.resid, g.ldr = ptr(resid), (resid.stride(0) if resid is not None else 0)
    g.addtab, g.tab_rows = ptr(addtab), (addtab.shape[0] if addtab is not None else 0)
    o2 = out[0] if (mode in _OUT_SPLIT or (not mode and np_ == 2)) else out
    g.out, g.ldo, g.out_f32 = ptr(out), o2.stride(0), mode
    g.out_plane = out[0].numel() if mode in _OUT_SPLIT else (0 if mode else operand.plane_offset(out, prec))
    g.w_qexp = int(w_qexp)
    if rms is not None:                      # (wq, wk, eps[, parts]): fused q/k RMSNorm of a QKV Linear ([q | k | v] columns, or [q | k])
        g.rms_wq, g.rms_wk, g.rms_eps = ptr(rms[0]), ptr(rms[1]), float(rms[2])
        g.rms_parts = int(rms[3]) if len(rms) > 3 else 0
    g.M, g.N, g.K, g.act = M, N, K, act
    g.rpg_in, g.rpg_out, g.row_off = rpg
    if ln_emit is not None:
        st, op = ln_emit
        g.ln_stats_out, g.ln_op_out, g.ln_op_plane, g.ln_op_ld = ptr(st), ptr(op), op[0].numel(), op[0].stride(0)
        g.ln_resid_in_op = int(bool(ln_resid_in_op))      # the residual rows are read from (and the sum written back to) `op`; fp32 rows only with out_f32
    if ln_apply is not None:
        g.ln_stats_in, g.ln_colsum, g.ln_eps = ptr(ln_apply[0]), ptr(ln_apply[1]), float(ln_apply[2])
    if split_k is not None:
        g.sk_ws, g.sk_split = ptr(split_k[0]), int(split_k[1])
    if (ln_emit is not None or ln_apply is not None) and not lib.bd_gemm_takes_ln_fold(C.byref(g), prec_id(prec)):
        raise ValueError("bd_gemm_takes_ln_fold: this launch has no kernel form with the LayerNorm-fold epilogues")
    if expect is not None:
        _check_expect(g, prec, expect)
    check(lib.bd_gemm(C.byref(g), prec_id(prec), stream()), "bd_gemm")
    return out


def splitk_workspace(M, N, device="cuda"):
    """Zeroed scratch region for gemm(..., split_k=(ws, factor)); None when (M, N) has no split-K form."""
    nbytes = _lib.load().bd_gemm_splitk_workspace_bytes(int(M), int(N))
    return torch.zeros(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def layernorm(x, gamma, beta, eps, *, prec="bf16", want16=True, want32=False, rows=None, rpg=(0, 0, 0)):
    lib = _lib.load()
    M = rows if rows is not None else x.shape[0]
    cols = x.shape[1]
    o16 = operand.empty(prec, M, cols, x.device) if want16 else None
    o32 = torch.empty((M, cols), dtype=torch.float32, device=x.device) if want32 else None
    check(lib.bd_layernorm(ptr(x), x.stride(0), ptr(gamma), ptr(beta), eps, ptr(o16),
                           operand.plane_offset(o16, prec) if o16 is not None else 0, ptr(o32), cols, M, cols, *rpg,
                           prec_id(prec), stream()), "bd_layernorm")
    return o16, o32


def qk_rmsnorm_(qkv16, wq, wk, eps, heads, head_dim, *, prec="bf16"):
    lib = _lib.load()
    q2 = qkv16[0] if planes(prec) == 2 else qkv16
    rows = q2.numel() // (3 * heads * head_dim)
    check(lib.bd_qk_rmsnorm(ptr(qkv16), operand.plane_offset(qkv16, prec), ptr(wq), ptr(wk), eps, rows, heads, head_dim,
                            prec_id(prec), stream()), "bd_qk_rmsnorm")
    return qkv16


_ATTN_ENTRY = {"plain": _lib.ATTN_ENTRY_PLAIN, "q": _lib.ATTN_ENTRY_Q, "prefix": _lib.ATTN_ENTRY_PREFIX, "varlen": _lib.ATTN_ENTRY_VARLEN}


def attention_plan(entry, *, prec="bf16", latency_forms=False, q_view=False, pointers=(0x7F0000001000, 0x7F0000002000, 0x7F0000003000), **fields):
    """bd_attention_plan (host only): the launch attention / attention_q / attention_prefix / attention_varlen (entry "plain", "q",
    "prefix", "varlen") makes of a call with these integer arguments (fields of bd_attn_call; q_view: whether one is given).  A dict:
    kernel ("tiled": attn_kernel, "pp": the ping-pong kernel attn_kernel_pp), waves, planes, head_dim, out_mode, vl, key, grid, block,
    q_len, q_off, out_rows.  pointers: (qkv, out, view_start) addresses, made-up aligned ones by default.  Raises HipLibraryError where
    the entry point refuses the call."""
    call, plan = _lib.AttnCall(entry=_ATTN_ENTRY[entry], has_q_view=int(bool(q_view)), prec=prec_id(prec), latency_forms=int(bool(latency_forms)), **fields), _lib.AttnPlan()
    check(_lib.load().bd_attention_plan(C.byref(call), *pointers, C.byref(plan)), "bd_attention_plan")
    l = plan.launch[0]
    k = list(l.key)
    d = {"key": k, "grid": l.grid, "block": l.block, "q_len": l.q_len, "q_off": l.q_off, "out_rows": l.out_rows}
    if l.family == _lib.ATTN_FAMILY_PP:
        d.update(kernel="pp", waves=8, planes=1, head_dim=k[1], out_mode=k[2], vl=bool(k[3]))
    else:
        d.update(kernel="tiled", waves=k[3], planes=k[1], head_dim=k[2], out_mode=k[4], vl=bool(k[5]))
    return d


def attention(qkv16, batch, seq, heads, head_dim, scale, *, prec="bf16"):
    lib = _lib.load()
    dev = qkv16.device
    out = operand.empty(prec, batch * seq, heads * head_dim, dev)
    check(lib.bd_attention(ptr(qkv16), operand.plane_offset(qkv16, prec), ptr(out), operand.plane_offset(out, prec), batch, seq, heads,
                           head_dim, scale, prec_id(prec), stream()), "bd_attention")
    return out


def attention_prefix(qkv16, batch, seq, heads, head_dim, scale, n_prefix, *, prec="bf16", prefix_queries=True, out=None):
    """bd_attention_prefix: patch queries in the tiled kernel, the n_prefix leading queries in a side launch (or skipped)."""
    lib = _lib.load()
    if out is None:
        out = operand.empty(prec, batch * seq, heads * head_dim, qkv16.device)
    check(lib.bd_attention_prefix(ptr(qkv16), operand.plane_offset(qkv16, prec), ptr(out), operand.plane_offset(out, prec), batch, seq, heads, head_dim, scale,
                                  n_prefix, int(bool(prefix_queries)), prec_id(prec), stream()), "bd_attention_prefix")
    return out


def attention_q(qkv16, batch, seq, heads, head_dim, scale, q_view, q_len, *, prec="bf16"):
    """Attention with queries restricted to rows [q_view[b]*q_len, +q_len) of each sequence; compact output."""
    lib = _lib.load()
    out = operand.empty(prec, batch * q_len, heads * head_dim, qkv16.device)
    check(lib.bd_attention_q(ptr(qkv16), operand.plane_offset(qkv16, prec), ptr(out), operand.plane_offset(out, prec), batch, seq, heads, head_dim,
                             scale, ptr(q_view), q_len, prec_id(prec), stream()), "bd_attention_q")
    return out


def attention_varlen(qkv16, view_counts, tokens_per_view, heads, head_dim, scale, *, prec="bf16", q_view=None, view_start=None):
    """bd_attention_varlen on a packed ragged batch: qkv16 holds sum(view_counts) * tokens_per_view token rows, sample b the next
    view_counts[b] views.  view_counts: HOST ints.  q_view (device int32 [B], view index inside the sample): only that view's rows are
    queries, compact output [B * tokens_per_view, heads * head_dim]; None: every row is a query, packed output.  view_start: the
    device int32 [B + 1] offsets when the caller already holds them (else built here from the counts)."""
    lib = _lib.load()
    counts = _lib.view_counts_list(view_counts)
    dev = qkv16.device
    if view_start is None:
        view_start = torch.tensor(_lib.view_starts(counts), dtype=torch.int32).to(dev)
    B, n_views = len(counts), sum(counts)
    out = operand.empty(prec, (B if q_view is not None else n_views) * tokens_per_view, heads * head_dim, dev)
    check(lib.bd_attention_varlen(ptr(qkv16), operand.plane_offset(qkv16, prec), ptr(out), operand.plane_offset(out, prec), ptr(view_start), B, n_views,
                                  max(counts) if counts else 0, tokens_per_view, heads, head_dim, scale, ptr(q_view), prec_id(prec),
                                  stream()), "bd_attention_varlen")
    return out


def gather_view_rows(bank16, bank_views, fresh16, n_fresh, src, out16, n_views, P, dim, *, prec, bank_plane=None, fresh_plane=None,
                     out_plane=None, bank32=None, fresh32=None, out32=None):
    """bd_gather_view_rows: out view v = bank view src[v] (src[v] >= 0) or fresh view -(src[v] + 1), whole views of one operand class,
    one launch.  bank16 / fresh16 / out16: operand tensors ([rows, dim], or [2, rows, dim] for the two-plane classes; the plane offsets
    default to each tensor's own plane size) -- either source may be None when its view count is 0.  src: device int32 [n_views].
    bank32 / fresh32 / out32: optional fp32 copies moved the same way.  Returns out16."""
    lib = _lib.load()
    pl = [(operand.plane_offset(t, prec) if t is not None else 0) if given is None else int(given)
          for t, given in ((bank16, bank_plane), (fresh16, fresh_plane), (out16, out_plane))]
    check(lib.bd_gather_view_rows(ptr(bank16), pl[0], int(bank_views), ptr(fresh16), pl[1], int(n_fresh), ptr(src), ptr(out16), pl[2],
                                  int(n_views), int(P), int(dim), prec_id(prec), ptr(bank32), ptr(fresh32), ptr(out32), stream()),
          "bd_gather_view_rows")
    return out16


def assemble_entry_tokens(bank_x, bank_views, rgb_fresh, n_fresh, pos, query_token, src, x_out, n_views, P, dim):
    """bd_assemble_entry_tokens: x_out view v = bank_x view src[v] (src[v] >= 0, moved as bits) or, for the fresh view f = -(src[v] + 1),
    (query_token + rgb_fresh[f]) + pos -- the decoder's entry token rows of a batch, one launch.  bank_x fp32 [bank_views, P, dim],
    rgb_fresh fp32 [n_fresh, P, dim] (either may be None when its view count is 0), pos fp32 [P, dim], query_token fp32 [dim], src
    device int32 [n_views], x_out fp32 [n_views, P, dim].  Returns x_out."""
    lib = _lib.load()
    check(lib.bd_assemble_entry_tokens(ptr(bank_x), int(bank_views), ptr(rgb_fresh), int(n_fresh), ptr(pos), ptr(query_token), ptr(src),
                                       ptr(x_out), int(n_views), int(P), int(dim), stream()), "bd_assemble_entry_tokens")
    return x_out


def decoder_entry_tokens(weights, bbox_feat, feats16, feats16_plane, x_out, workspace, *, prec):
    """bd_decoder_entry_tokens: the decoder-entry token rows of free-standing views.  weights: the decoder's _lib.BetrWeights struct;
    bbox_feat [n_views, 8, S, S] (bf16 / fp16 / fp32, contiguous); feats16: the encoder's operand copy of the same views in the class
    of the adapter's first Linear (plane offset feats16_plane); x_out: fp32 [n_views * P, dim]; workspace: a uint8 tensor of at least
    bd_decoder_entry_tokens_workspace_bytes(weights, n_views, prec) bytes.  Returns x_out."""
    lib = _lib.load()
    if bbox_feat.dim() != 4 or not bbox_feat.is_contiguous() or x_out.dtype != torch.float32 or not x_out.is_contiguous():
        raise ValueError("decoder_entry_tokens needs contiguous (n_views, 8, S, S) heat maps and a contiguous fp32 output")
    n_views, size = int(bbox_feat.shape[0]), int(bbox_feat.shape[-1])
    if x_out.numel() != n_views * weights.grid * weights.grid * weights.dim:
        raise ValueError(f"x_out holds {x_out.numel()} elements, {n_views} views need {n_views * weights.grid * weights.grid * weights.dim}")
    check(lib.bd_decoder_entry_tokens(weights, ptr(bbox_feat), _lib.dtype_id(bbox_feat), ptr(feats16), int(feats16_plane), n_views, size,
                                      ptr(x_out), ptr(workspace), workspace.numel(), prec_id(prec), stream()), "bd_decoder_entry_tokens")
    return x_out


def match_view_sums(feats, images, threshold, sums=None, counts=None):
    """bd_match_view_sums: feats fp32 (V, L, D), images (V, 3, H, W) -> (sums fp32 (V, D), counts fp32 (V,)): each view's foreground
    feature sum and patch count, what a pair's dense-reference score is made of (csrc/match.hip).  `sums` / `counts`: where to write
    them (contiguous views of at least V rows), allocated when None."""
    lib = _lib.load()
    V, L, D = feats.shape
    H, W = images.shape[-2:]
    if feats.dtype != torch.float32 or not feats.is_contiguous() or not images.is_contiguous() or images.shape[0] != V:
        raise ValueError("match_view_sums needs contiguous fp32 (V, L, D) features and contiguous (V, 3, H, W) images of the same V")
    if sums is None:
        sums = torch.empty((V, D), dtype=torch.float32, device=feats.device)
        counts = torch.empty((V,), dtype=torch.float32, device=feats.device)
    check(lib.bd_match_view_sums(ptr(feats), ptr(images), _lib.dtype_id(images), int(V), int(L), int(D), int(H), int(W), float(threshold),
                                 ptr(sums), ptr(counts), stream()), "bd_match_view_sums")
    return sums, counts


def match_select_rows(bank_sums, bank_counts, n_bank, q_sums, q_counts, rows, n_refs, L, k):
    """bd_match_select_rows: one launch -> (scores fp32 (B, N_max), sel int32 (B, k), src int32 (B * (k + 1),)).  rows: device int32
    (B, N_max) bank row of every reference slot; n_refs: device int32 (B,); n_bank: rows of the bank that are in use."""
    lib = _lib.load()
    B, N_max = rows.shape
    D = q_sums.shape[1]
    dev = q_sums.device
    scores = torch.empty((B, N_max), dtype=torch.float32, device=dev)
    sel = torch.empty((B, int(k)), dtype=torch.int32, device=dev)
    src = torch.empty((B * (int(k) + 1),), dtype=torch.int32, device=dev)
    check(lib.bd_match_select_rows(ptr(bank_sums), ptr(bank_counts), int(n_bank), ptr(q_sums), ptr(q_counts), ptr(rows), ptr(n_refs),
                                   int(B), int(N_max), int(L), int(D), int(k), ptr(scores), ptr(sel), ptr(src), stream()),
          "bd_match_select_rows")
    return scores, sel, src


def round_sources(rows, cand, n_bank, sub, zero_row, per_round_query):
    """bd_round_sources: one launch -> (src, view), both int32 (B * R * (sub + 1),), R = ceil(k / sub): the source table of the
    (B * R, sub + 1) multi-round batch and each entry's view position in the filtered (B, k + 1) batch (-1: zero padding).  rows:
    device int32 (B, N_max); cand: device int32 (B, k), bd_match_select_rows' sel; n_bank: rows of the bank that are in use (the
    zero row among them); zero_row: the bank's all-zero view, -1 when no round is padded."""
    lib = _lib.load()
    (B, N_max), k, sub = rows.shape, int(cand.shape[1]), int(sub)
    if rows.dtype != torch.int32 or cand.dtype != torch.int32 or cand.shape[0] != B or not rows.is_contiguous() or not cand.is_contiguous():
        raise ValueError("round_sources needs contiguous int32 rows (B, N_max) and cand (B, k) of the same B")
    n = B * (-(-k // sub) if sub > 0 else 0) * (sub + 1)
    src = torch.empty((max(n, 0),), dtype=torch.int32, device=rows.device)
    view = torch.empty_like(src)
    check(lib.bd_round_sources(ptr(rows), ptr(cand), int(n_bank), int(B), int(N_max), k, sub, int(zero_row), int(bool(per_round_query)),
                               ptr(src), ptr(view), stream()), "bd_round_sources")
    return src, view


def pose_select_rows(bank_poses, n_bank, pred, rows, cand, fk):
    """bd_pose_select_rows: one launch -> (dist fp32 (B, k), fine_pos int32 (B, fk), src int32 (B * (fk + 1),)).  bank_poses: fp32
    (capacity, 4, 4), n_bank rows in use; pred: fp32 (B, 4, 4) coarse poses; rows / cand: as round_sources."""
    lib = _lib.load()
    (B, N_max), k, fk = rows.shape, int(cand.shape[1]), int(fk)
    if (bank_poses.dtype != torch.float32 or pred.dtype != torch.float32 or not bank_poses.is_contiguous() or not pred.is_contiguous()
            or tuple(bank_poses.shape[1:]) != (4, 4) or tuple(pred.shape) != (B, 4, 4) or bank_poses.shape[0] < int(n_bank)):
        raise ValueError("pose_select_rows needs contiguous fp32 bank_poses (>= n_bank, 4, 4) and pred (B, 4, 4)")
    if rows.dtype != torch.int32 or cand.dtype != torch.int32 or cand.shape[0] != B or not rows.is_contiguous() or not cand.is_contiguous():
        raise ValueError("pose_select_rows needs contiguous int32 rows (B, N_max) and cand (B, k) of the same B")
    dev = pred.device
    dist = torch.empty((B, k), dtype=torch.float32, device=dev)
    fine_pos = torch.empty((B, max(fk, 0)), dtype=torch.int32, device=dev)
    src = torch.empty((B * (max(fk, 0) + 1),), dtype=torch.int32, device=dev)
    check(lib.bd_pose_select_rows(ptr(bank_poses), int(n_bank), ptr(pred), ptr(rows), ptr(cand), int(B), int(N_max), k, fk, ptr(dist),
                                  ptr(fine_pos), ptr(src), stream()), "bd_pose_select_rows")
    return dist, fine_pos, src


def im2col_images(images, patch=14, kpad=640, *, prec="bf16"):
    lib = _lib.load()
    images = images.contiguous()
    n, size = images.shape[0], images.shape[-1]
    grid = size // patch
    out = operand.empty(prec, n * grid * grid, kpad, images.device)
    check(lib.bd_im2col_images(ptr(images), _lib.dtype_id(images), ptr(out), operand.plane_offset(out, prec), n, size, patch,
                               kpad, prec_id(prec), stream()), "bd_im2col_images")
    return out


def patchify_heatmaps(heat, patch=14, kpad=1600, *, prec="bf16"):
    lib = _lib.load()
    heat = heat.contiguous()
    n, c, size = heat.shape[0], heat.shape[1], heat.shape[-1]
    grid = size // patch
    out = operand.empty(prec, n * grid * grid, kpad, heat.device)
    check(lib.bd_patchify_heatmaps(ptr(heat), _lib.dtype_id(heat), ptr(out), operand.plane_offset(out, prec), n, c, size, patch,
                                   kpad, prec_id(prec), stream()), "bd_patchify_heatmaps")
    return out


def unpatchify_sigmoid(proj, B, size=224, patch=14):
    lib = _lib.load()
    logits = torch.empty((B, 8, size, size), dtype=torch.float32, device=proj.device)
    heat = torch.empty_like(logits)
    check(lib.bd_unpatchify_sigmoid(ptr(proj), ptr(logits), ptr(heat), B, 8, size, patch, stream()),
          "bd_unpatchify_sigmoid")
    return logits, heat


def decode_topk(heat, k=20, want_idx=True):
    """heat: fp32 [..., H, W] in [-1, 1] -> (kp_px [..., 2], kp_norm [..., 2], idx [..., k] int32)."""
    lib = _lib.load()
    heat = heat.contiguous()
    if heat.dtype != torch.float32:
        heat = heat.float()
    H, W = heat.shape[-2:]
    lead = heat.shape[:-2]
    n = heat.numel() // (H * W)
    kp = torch.empty((n, 2), dtype=torch.float32, device=heat.device)
    kn = torch.empty_like(kp)
    idx = torch.empty((n, k), dtype=torch.int32, device=heat.device) if want_idx else None
    check(lib.bd_decode_topk(ptr(heat), n, H, W, k, ptr(kp), ptr(kn), ptr(idx), stream()), "bd_decode_topk")
    return kp.reshape(*lead, 2), kn.reshape(*lead, 2), (idx.reshape(*lead, k) if want_idx else None)


def _stream_dev(t, shape, dtype, name):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got "
                         f"{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}")
    return t


def stream_windows(det_boxes, K, padding=0.1, out_size=224, windows=None, K_crop=None):
    """bd_stream_windows: det_boxes fp32 (n, 4) x0 y0 x1 y1, K fp32 (n, 3, 3) of the full frame -> (windows int32 (n, 4), K_crop fp32
    (n, 3, 3)): preprocess.square_bbox(det_boxes, padding) and preprocess.crop_intrinsics(K, windows, out_size) in ONE launch, bit for
    bit.  `windows` / `K_crop`: where to write them (allocated when None)."""
    lib = _lib.load()
    n = int(det_boxes.shape[0]) if isinstance(det_boxes, torch.Tensor) and det_boxes.dim() == 2 else -1
    _stream_dev(det_boxes, (n, 4), torch.float32, "det_boxes")
    _stream_dev(K, (n, 3, 3), torch.float32, "K")
    windows = torch.empty((n, 4), dtype=torch.int32, device=det_boxes.device) if windows is None else _stream_dev(windows, (n, 4), torch.int32, "windows")
    K_crop = torch.empty((n, 3, 3), dtype=torch.float32, device=det_boxes.device) if K_crop is None else _stream_dev(K_crop, (n, 3, 3), torch.float32, "K_crop")
    _lib.same_device(det_boxes, K, windows, K_crop)
    check(lib.bd_stream_windows(ptr(det_boxes), ptr(K), float(padding), int(out_size), ptr(windows), ptr(K_crop), n, stream()), "bd_stream_windows")
    return windows, K_crop


def stream_track_windows(prev_rows, bbox_3d, K, det_boxes, det_valid, force, state_box, padding=0.1, out_size=224, frame_shape=(480, 640),
                         max_rms_px=float("inf"), min_side_px=8.0, max_side_px=None, windows=None, K_crop=None, box_src=None,
                         keep_boxes=None, track=None):
    """bd_stream_track_windows: one launch -> (windows int32 (n, 4), K_crop fp32 (n, 3, 3), box_src int32 (n,)); `state_box` fp32 (n, 4)
    is read and UPDATED IN PLACE with the box used.  prev_rows fp32 (n, 66): the last step's result rows; bbox_3d fp32 (n, 8, 3); K fp32
    (n, 3, 3) of the full frame; det_boxes fp32 (n, 4); det_valid / force int32 (n,); frame_shape (H, W); max_side_px None: 4 x
    max(H, W).  keep_boxes int32 (n, 4) / track fp32 (n, 5): written when given (the truncated box; x0 y0 x1 y1 src).  The rule:
    include/boxdreamer_hip.h."""
    lib = _lib.load()
    n = int(prev_rows.shape[0]) if isinstance(prev_rows, torch.Tensor) and prev_rows.dim() == 2 else -1
    frame_h, frame_w = (int(x) for x in frame_shape)
    max_side_px = 4.0 * max(frame_h, frame_w) if max_side_px is None else float(max_side_px)
    _stream_dev(prev_rows, (n, _lib.STREAM_ROW_FLOATS), torch.float32, "prev_rows")
    _stream_dev(bbox_3d, (n, 8, 3), torch.float32, "bbox_3d")
    _stream_dev(K, (n, 3, 3), torch.float32, "K")
    _stream_dev(det_boxes, (n, 4), torch.float32, "det_boxes")
    _stream_dev(det_valid, (n,), torch.int32, "det_valid")
    _stream_dev(force, (n,), torch.int32, "force")
    _stream_dev(state_box, (n, 4), torch.float32, "state_box")
    dev = prev_rows.device
    windows = torch.empty((n, 4), dtype=torch.int32, device=dev) if windows is None else _stream_dev(windows, (n, 4), torch.int32, "windows")
    K_crop = torch.empty((n, 3, 3), dtype=torch.float32, device=dev) if K_crop is None else _stream_dev(K_crop, (n, 3, 3), torch.float32, "K_crop")
    box_src = torch.empty((n,), dtype=torch.int32, device=dev) if box_src is None else _stream_dev(box_src, (n,), torch.int32, "box_src")
    if keep_boxes is not None:
        _stream_dev(keep_boxes, (n, 4), torch.int32, "keep_boxes")
    if track is not None:
        _stream_dev(track, (n, 5), torch.float32, "track")
    _lib.same_device(prev_rows, bbox_3d, K, det_boxes, det_valid, force, state_box, windows, K_crop, box_src, keep_boxes, track)
    check(lib.bd_stream_track_windows(ptr(prev_rows), ptr(bbox_3d), ptr(K), ptr(det_boxes), ptr(det_valid), ptr(force), ptr(state_box),
                                      float(padding), int(out_size), frame_h, frame_w, float(max_rms_px), float(min_side_px), max_side_px,
                                      ptr(windows), ptr(K_crop), ptr(box_src), ptr(keep_boxes), ptr(track), n, stream()),
          "bd_stream_track_windows")
    return windows, K_crop, box_src


def stream_results(poses, rms_px, kp_px, windows, K, bbox_3d, out_size=224, rows=None):
    """bd_stream_results: poses fp32 (n, 4, 4), rms_px fp32 (n,), kp_px fp32 (n, 8, 2), windows int32 (n, 4), K fp32 (n, 3, 3) of the
    full frame, bbox_3d fp32 (n, 8, 3) -> rows fp32 (n, 66) in ONE launch (the layout: include/boxdreamer_hip.h), written into `rows`
    when given."""
    lib = _lib.load()
    n = int(poses.shape[0]) if isinstance(poses, torch.Tensor) and poses.dim() == 3 else -1
    _stream_dev(poses, (n, 4, 4), torch.float32, "poses")
    _stream_dev(rms_px, (n,), torch.float32, "rms_px")
    _stream_dev(kp_px, (n, 8, 2), torch.float32, "kp_px")
    _stream_dev(windows, (n, 4), torch.int32, "windows")
    _stream_dev(K, (n, 3, 3), torch.float32, "K")
    _stream_dev(bbox_3d, (n, 8, 3), torch.float32, "bbox_3d")
    shape = (n, _lib.STREAM_ROW_FLOATS)
    rows = torch.empty(shape, dtype=torch.float32, device=poses.device) if rows is None else _stream_dev(rows, shape, torch.float32, "rows")
    _lib.same_device(poses, rms_px, kp_px, windows, K, bbox_3d, rows)
    check(lib.bd_stream_results(ptr(poses), ptr(rms_px), ptr(kp_px), ptr(windows), ptr(K), ptr(bbox_3d), int(out_size), ptr(rows), n, stream()),
          "bd_stream_results")
    return rows


def stream_select_rows(sums, counts, poses, n_rows, q_sums, q_counts, prev_rows, rows, n_refs, force, L, k, rule, max_rms_px=float("inf"),
                       scores=None, dist=None, used=None, sel=None, src=None):
    """bd_stream_select_rows: one launch -> (scores fp32 (B, N_max), dist fp32 (B, N_max) or None, used int32 (B,), sel int32 (B, k),
    src int32 (B * (k + 1),)).  sums fp32 (>= n_rows, D) / counts fp32 (>= n_rows,) / poses fp32 (>= n_rows, 4, 4) or None (rule
    _lib.STREAM_SELECT_DINO only; dist is then None): the database views' match summaries and poses, n_rows of them in use; q_sums (B, D)
    / q_counts (B,): match_view_sums of the query crops; prev_rows fp32 (B, 66): the previous step's result rows; rows int32
    (B, N_max) / n_refs int32 (B,) / force int32 (B,): device tables.  The outputs are written into the given tensors, allocated when
    None."""
    lib = _lib.load()
    B, N_max = (int(x) for x in rows.shape) if isinstance(rows, torch.Tensor) and rows.dim() == 2 else (-1, -1)
    k, n_rows = int(k), int(n_rows)
    D = int(q_sums.shape[1]) if isinstance(q_sums, torch.Tensor) and q_sums.dim() == 2 else -1
    _stream_dev(rows, (B, N_max), torch.int32, "rows")
    _stream_dev(n_refs, (B,), torch.int32, "n_refs")
    _stream_dev(force, (B,), torch.int32, "force")
    _stream_dev(q_sums, (B, D), torch.float32, "q_sums")
    _stream_dev(q_counts, (B,), torch.float32, "q_counts")
    _stream_dev(prev_rows, (B, _lib.STREAM_ROW_FLOATS), torch.float32, "prev_rows")
    for t, tail, name in ((sums, (D,), "sums"), (counts, (), "counts"), (poses, (4, 4), "poses")):
        if t is None and name == "poses":
            continue
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape[1:]) != tail
                or t.shape[0] < n_rows):
            raise ValueError(f"{name} must be a contiguous fp32 tensor of shape (>= {n_rows},) + {tail}, got "
                             f"{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}")
    dev = rows.device
    kk = max(k, 0)
    outs = []
    for t, shape, dtype, name in ((scores, (B, N_max), torch.float32, "scores"), (dist, (B, N_max), torch.float32, "dist"),
                                  (used, (B,), torch.int32, "used"), (sel, (B, kk), torch.int32, "sel"),
                                  (src, (B * (kk + 1),), torch.int32, "src")):
        if name == "dist" and poses is None:
            outs.append(None)
        else:
            outs.append(torch.empty(shape, dtype=dtype, device=dev) if t is None else _stream_dev(t, shape, dtype, name))
    scores, dist, used, sel, src = outs
    _lib.same_device(sums, counts, poses, q_sums, q_counts, prev_rows, rows, n_refs, force, scores, dist, used, sel, src)
    check(lib.bd_stream_select_rows(ptr(sums), ptr(counts), ptr(poses), n_rows, ptr(q_sums), ptr(q_counts), ptr(prev_rows), ptr(rows),
                                    ptr(n_refs), ptr(force), B, N_max, int(L), D, k, int(rule), float(max_rms_px), ptr(scores), ptr(dist),
                                    ptr(used), ptr(sel), ptr(src), stream()), "bd_stream_select_rows")
    return scores, dist, used, sel, src


def _host32(a, shape, dtype):
    import numpy as np
    a = np.ascontiguousarray(a.numpy() if isinstance(a, torch.Tensor) else a, dtype=dtype)
    if a.shape != tuple(shape):
        raise ValueError(f"expected a host array of shape {tuple(shape)}, got {a.shape}")
    return a


def stream_windows_host(det_boxes, K, padding=0.1, out_size=224):
    """bd_stream_windows_host: the same arithmetic on host arrays (numpy or CPU tensors) -> (windows int32 (n, 4), K_crop fp32 (n, 3, 3)),
    numpy.  Needs no GPU."""
    import numpy as np
    lib = _lib.load()
    n = len(det_boxes)
    b, k = _host32(det_boxes, (n, 4), np.float32), _host32(K, (n, 3, 3), np.float32)
    windows, K_crop = np.empty((n, 4), np.int32), np.empty((n, 3, 3), np.float32)
    rc = lib.bd_stream_windows_host(b.ctypes.data, k.ctypes.data, float(padding), int(out_size), windows.ctypes.data, K_crop.ctypes.data, n)
    check(rc, "bd_stream_windows_host")
    return windows, K_crop


def stream_track_windows_host(prev_rows, bbox_3d, K, det_boxes, det_valid, force, state_box, padding=0.1, out_size=224,
                              frame_shape=(480, 640), max_rms_px=float("inf"), min_side_px=8.0, max_side_px=None, want_keep=False):
    """bd_stream_track_windows_host: the same arithmetic on host arrays (numpy or CPU tensors) -> a dict of numpy arrays: windows int32
    (n, 4), K_crop fp32 (n, 3, 3), state_box fp32 (n, 4) (the UPDATED boxes: the input is not touched), box_src int32 (n,), track fp32
    (n, 5) and, with want_keep, keep_boxes int32 (n, 4).  Needs no GPU."""
    import numpy as np
    lib = _lib.load()
    n = len(prev_rows)
    frame_h, frame_w = (int(x) for x in frame_shape)
    max_side_px = 4.0 * max(frame_h, frame_w) if max_side_px is None else float(max_side_px)
    args = (_host32(prev_rows, (n, _lib.STREAM_ROW_FLOATS), np.float32), _host32(bbox_3d, (n, 8, 3), np.float32), _host32(K, (n, 3, 3), np.float32),
            _host32(det_boxes, (n, 4), np.float32), _host32(det_valid, (n,), np.int32), _host32(force, (n,), np.int32))
    state = _host32(state_box, (n, 4), np.float32).copy()
    out = dict(windows=np.empty((n, 4), np.int32), K_crop=np.empty((n, 3, 3), np.float32), state_box=state, box_src=np.empty((n,), np.int32),
               track=np.empty((n, 5), np.float32))
    keep = np.empty((n, 4), np.int32) if want_keep else None
    rc = lib.bd_stream_track_windows_host(*(a.ctypes.data for a in args), state.ctypes.data, float(padding), int(out_size), frame_h, frame_w,
                                          float(max_rms_px), float(min_side_px), max_side_px, out["windows"].ctypes.data,
                                          out["K_crop"].ctypes.data, out["box_src"].ctypes.data, keep.ctypes.data if want_keep else None,
                                          out["track"].ctypes.data, n)
    check(rc, "bd_stream_track_windows_host")
    if want_keep:
        out["keep_boxes"] = keep
    return out


def stream_results_host(poses, rms_px, kp_px, windows, K, bbox_3d, out_size=224):
    """bd_stream_results_host: the same arithmetic on host arrays (numpy or CPU tensors) -> rows fp32 (n, 66), numpy.  Needs no GPU."""
    import numpy as np
    lib = _lib.load()
    n = len(poses)
    args = (_host32(poses, (n, 4, 4), np.float32), _host32(rms_px, (n,), np.float32), _host32(kp_px, (n, 8, 2), np.float32),
            _host32(windows, (n, 4), np.int32), _host32(K, (n, 3, 3), np.float32), _host32(bbox_3d, (n, 8, 3), np.float32))
    rows = np.empty((n, _lib.STREAM_ROW_FLOATS), np.float32)
    rc = lib.bd_stream_results_host(*(a.ctypes.data for a in args), int(out_size), rows.ctypes.data, n)
    check(rc, "bd_stream_results_host")
    return rows
