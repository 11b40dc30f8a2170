#!/usr/bin/env python3
"""NF4 vs FP4 on one MI355X: per-launch HIP-event microseconds of dequant, batch-1 GEMV, NF4 dequant + hipBLASLt at batch 1 and the
quantiser, at the decoder shapes; the GEMV's two LDS-table layouts (fp4_hip_set_variant("gemv_nf4", 0 / 1)); and a steady-state
NF4 GEMV over a stack of distinct weights (no cache reuse) as a fraction of 8 TB/s.  Prints one JSON line.

Timing as bench.py does it (its capture / time_replays helpers): R launches captured in one HIP graph, the median over replays,
divided by R.  usage: python tools/nf4_bench.py [--reps 20] [--launches 20]

--small-batch: the 2..16-row regime instead (profiles/nf4_small_batch.json).  Per dtype (bf16, fp16), shape and row count
(2 / 4 / 8 / 16), in one run on the same operands: (a) gemm_small_nf4, the fused matrix-core kernel; (b) qlinear_nf4, NF4 dequant +
hipBLASLt - what these calls cost without the switch; (c) gemm_small_fp4 on the same bytes (the price of the NF4 decode and of the
doubled matrix work); (d) gemv_nf4 once per row.  (a) and (b) also carry min / max / p10 / p90 over the replays, and each cell says
whether (a) beats (b) by more than the two full ranges (max - min) together.

--wide-batch: the 17..128-row regime (profiles/nf4_wide_batch.json).  Per dtype, shape (the four decoder shapes and 4096 x 11008)
and row count (17 / 32 / 48 / 64 / 96 / 128; K = 11008 also 2 / 8 / 16), in one run on the same operands: (a) gemm_wide_nf4, the
one-pass kernel, under its own heuristic and with 16 / 32 weight rows per workgroup forced (fp4_hip_set_variant("gemm_wide_nf4",
1 / 2)); (b) qlinear_nf4; (c) ceil(rows / 16) launches of gemm_small_nf4 (K % 512 == 0 only); (d) gemm_small_fp4 on the same
bytes, for orientation.  (a), (b), (c) carry min / max over the replays; a cell is won where (a) beats (b) AND (c), each by more than
the two full ranges together.  --revision names the tree the figures belong to.

--fused: the decode epilogues (profiles/nf4_fused_epilogues.json), bf16, one run on the same operands.  (1) The plain calls the
epilogue work touched - gemv_nf4, gemm_small_nf4 at 2 / 16 rows, gemm_wide_nf4 at 32 / 64 rows, 4096 x 4096 and 14336 x 4096 - through
this tree's library and, with --baseline-lib, through another build of it (the parent commit's) loaded side by side; a cell is
"within" where the medians differ by no more than the larger of the two replay-to-replay ranges.  (2) The fused ops against the
unfused sequence they replace (the plain op, then torch's silu / mul / add) at the Mistral-7B shapes and 1 / 8 / 32 / 64 rows: the
o projection with its residual add, gate|up with silu(g) * u, and gate|up + down with the residual; a cell is won where the fused
form is ahead by more than both ranges together.

--lora: LoRA adapters beside NF4 weights (profiles/nf4_lora.json), the four decoder shapes, 1 / 8 / 32 / 64 rows, rank 16 / 64, bf16 and
fp16, one run on the same operands, all through the torch ops as the layers issue them: (a) lora_down + gemv_nf4_lora / gemm_nf4_lora;
(b) the parent's best - the fused NF4 op plus the adapter as torch ops in the activation dtype, ((x @ A^T) * s) @ B^T and an add;
(c) the fused NF4 op alone (what the adapter costs on top).  The 28672-row shape runs the gate|up epilogue, where (b) has to take the
plain rows, add and apply silu * up itself.  A cell is won where (a) is ahead of (b) by more than both replay-to-replay ranges together.
--lora-ranks / --lora-rows replace the rank and row lists.

--multi-lora: several adapters in one batch (profiles/nf4_multi_lora.json), bf16, the four decoder shapes, 8 / 32 / 64 rows, rank 16 /
64, 1 / 4 / 8 distinct adapters in the batch with the ids sorted and interleaved, one run on the same operands, the protocol of --lora.
(a) lora_down_multi + gemm_nf4_lora_multi over a stack of 8 adapters; (b) the best a single-adapter layer offers for a mixed batch:
rows grouped by adapter on the host and, per group, index_select -> LoRANF4Linear -> index_copy; with one distinct adapter (b) is the
single-adapter fused pair itself, so that column shows what the indirection alone costs.  A cell is ahead / level / behind by more
than both replay-to-replay ranges together.  With --baseline-lib the plain and the single-adapter entry points (gemv_fused_nf4,
gemm_fused_nf4, lora_down, gemm_lora_nf4) also run through another build of the library (the parent commit's) side by side; "within"
as for --fused.

--nested: double-quantised absmax (profiles/nf4_nested.json), bf16, the four decoder shapes, one run on the same operands, the
protocol of --fused.  (1) fp4_hip_gemv_nested_nf4 on the compressed statistics against fp4_hip_gemv_fused_nf4 on their expansion
(level / ahead / behind beyond both replay-to-replay ranges).  (2) The plain fp4_hip_gemv_nf4 of this tree's library and, with
--baseline-lib, of the parent commit's, side by side; "within" as for --fused.  (3) absmax_unnest alone, and qlinear_nf4_nested
against qlinear_nf4 at 8 and 64 rows.  (4) Device bytes of one layer's statistics, resident and expanded.  (5) 2 / 8 / 16 / 32 / 64 rows:
gemm_nf4_nested against the parent commit's path for the same resident layer (qlinear_nf4_nested), both through the torch ops; and
fp4_hip_gemm_nested_nf4 against fp4_hip_gemm_fused_nf4 on the expanded statistics (this tree's library and the baseline's).  (6) A
rank-16 adapter at 1 / 8 / 32 rows: lora_down + gemv_nf4_lora_nested / gemm_nf4_lora_nested against the parent's resident path plus the
adapter as torch ops; and the C entry points against lora_down + the un-nested LoRA forms on expanded statistics.  A cell is "ahead"
only beyond both replay-to-replay ranges together.  --nested-rows / --nested-lora-rows replace the row lists.
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "torch-bnb-fp4_amd")]

import torch  # noqa: E402

import torch_bnb_fp4 as pkg  # noqa: E402
from bench import capture, time_replays  # noqa: E402

SHAPES = [(4096, 4096), (14336, 4096), (4096, 14336), (28672, 4096)]
DT = {torch.float16: 0, torch.float32: 1, torch.bfloat16: 2}
NAME = {torch.float16: "fp16", torch.float32: "f32", torch.bfloat16: "bf16"}
TREE, NF4 = 1, 2
BS = 64
SPEC_BPS = 8e12


def lib():
    l = ctypes.CDLL(pkg.HIP_LIBRARY_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    l.fp4_hip_dequantize_blockwise.argtypes = [vp, vp, vp, i32, i64, i32, i32, i32, vp]
    for g in (l.fp4_hip_gemv, l.fp4_hip_gemv_nf4):
        g.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp]
    for q in (l.fp4_hip_quantize_blockwise, l.fp4_hip_quantize_blockwise_nf4):
        q.argtypes = [vp, i32, vp, vp, i64, i32, vp]
    l.fp4_hip_set_variant.argtypes = [ctypes.c_char_p, i32]
    return l


def small_batch(args):
    L = lib()
    L.fp4_hip_gemm_small_nf4.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
    dev = torch.device("cuda", 0)
    s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def check(rc):
        if rc:
            raise RuntimeError(L.fp4_hip_last_error().decode())

    def timed(fn):
        replay = capture(lambda: [fn() for _ in range(args.launches)])
        med, samples = time_replays(replay, args.reps, args.launches)
        q = sorted(samples)
        return {"us": round(med, 2), "min_us": round(q[0], 2), "max_us": round(q[-1], 2), "p10_us": round(q[len(q) // 10], 2),
                "p90_us": round(q[-1 - len(q) // 10], 2)}

    cells = []
    for M, K in SHAPES:
        n = M * K
        torch.manual_seed(0)
        w16 = (torch.randn(n, device=dev) * 0.02).to(torch.float16)
        packed = torch.empty(n // 2, dtype=torch.uint8, device=dev)
        absmax = torch.empty(n // BS, dtype=torch.float32, device=dev)
        check(L.fp4_hip_quantize_blockwise_nf4(p_(w16), DT[torch.float16], p_(packed), p_(absmax), n, BS, s()))
        del w16
        B_t = packed.view(-1, 1).t()
        for dtype in (torch.bfloat16, torch.float16):
            for rows in (2, 4, 8, 16):
                x = torch.randn(rows, K, device=dev).to(dtype)
                y = torch.empty(rows, M, dtype=dtype, device=dev)
                a = timed(lambda: check(L.fp4_hip_gemm_small_nf4(p_(x), p_(packed), p_(absmax), None, p_(y), rows, M, K, BS, DT[dtype], s())))
                b = timed(lambda: pkg.ext.qlinear_nf4(x, packed, absmax, M, K, BS))
                c = timed(lambda: pkg.ext.gemm_small_fp4(x, B_t, absmax, BS, [M, K], None))
                d = timed(lambda: [check(L.fp4_hip_gemv_nf4(p_(x[i]), p_(packed), p_(absmax), None, p_(y[i]), M, K, BS, DT[dtype], s()))
                                   for i in range(rows)])
                # the torch op on the same call, as QuantData issues it (allocation of the output included)
                a_op = timed(lambda: pkg.ext.gemm_small_nf4(x, B_t, absmax, BS, [M, K], None))
                spread = (a["max_us"] - a["min_us"]) + (b["max_us"] - b["min_us"])
                cells.append({"M": M, "K": K, "dtype": NAME[dtype], "rows": rows, "gemm_small_nf4": a, "gemm_small_nf4_torch_op_us": a_op["us"],
                              "qlinear_nf4": b, "gemm_small_fp4_us": c["us"], "gemv_nf4_x_rows_us": d["us"],
                              "speedup_vs_qlinear_nf4": round(b["us"] / a["us"], 2), "nf4_over_fp4": round(a["us"] / c["us"], 3),
                              "vs_gemv_x_rows": round(a["us"] / d["us"], 3), "spread_us": round(spread, 2),
                              "beats_qlinear_nf4_beyond_spread": bool(b["us"] - a["us"] > spread)})
        del packed, absmax
    print(json.dumps({"device": torch.cuda.get_device_name(0), "blocksize": BS, "launches_per_graph": args.launches, "reps": args.reps,
                      "all_cells_beat_qlinear_nf4": all(c["beats_qlinear_nf4_beyond_spread"] for c in cells), "cells": cells}))


WIDE_SHAPES = SHAPES + [(4096, 11008)]


def wide_batch(args):
    L = lib()
    sig = [ctypes.c_void_p] * 5 + [ctypes.c_int64] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
    L.fp4_hip_gemm_small_nf4.argtypes = sig
    L.fp4_hip_gemm_wide_nf4.argtypes = sig
    dev = torch.device("cuda", 0)
    s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def check(rc):
        if rc:
            raise RuntimeError(L.fp4_hip_last_error().decode())

    def timed(fn):
        replay = capture(lambda: [fn() for _ in range(args.launches)])
        med, samples = time_replays(replay, args.reps, args.launches)
        q = sorted(samples)
        return {"us": round(med, 2), "min_us": round(q[0], 2), "max_us": round(q[-1], 2)}

    def beyond(new, base):  # new beats base by more than the two replay-to-replay ranges together
        spread = (new["max_us"] - new["min_us"]) + (base["max_us"] - base["min_us"])
        return bool(base["us"] - new["us"] > spread)

    cells = []
    for M, K in WIDE_SHAPES:
        n = M * K
        torch.manual_seed(0)
        w16 = (torch.randn(n, device=dev) * 0.02).to(torch.float16)
        packed = torch.empty(n // 2, dtype=torch.uint8, device=dev)
        absmax = torch.empty(n // BS, dtype=torch.float32, device=dev)
        check(L.fp4_hip_quantize_blockwise_nf4(p_(w16), DT[torch.float16], p_(packed), p_(absmax), n, BS, s()))
        del w16
        B_t = packed.view(-1, 1).t()
        for dtype in (torch.bfloat16, torch.float16):
            for rows in ([2, 8, 16] if K % 512 else []) + [17, 32, 48, 64, 96, 128]:
                x = torch.randn(rows, K, device=dev).to(dtype)
                y = torch.empty(rows, M, dtype=dtype, device=dev)
                wide = lambda: check(L.fp4_hip_gemm_wide_nf4(p_(x), p_(packed), p_(absmax), None, p_(y), rows, M, K, BS, DT[dtype], s()))  # noqa: E731
                a = timed(wide)
                forced = {}
                for v in (1, 2):
                    L.fp4_hip_set_variant(b"gemm_wide_nf4", v)
                    forced[v] = timed(wide)["us"]
                L.fp4_hip_set_variant(b"gemm_wide_nf4", -1)
                b = timed(lambda: pkg.ext.qlinear_nf4(x, packed, absmax, M, K, BS))
                cell = {"M": M, "K": K, "dtype": NAME[dtype], "rows": rows, "gemm_wide_nf4": a, "rows16_per_workgroup_us": forced[1],
                        "rows32_per_workgroup_us": forced[2], "qlinear_nf4": b, "speedup_vs_qlinear_nf4": round(b["us"] / a["us"], 2)}
                won = beyond(a, b)
                if K % 512 == 0:
                    c = timed(lambda: [check(L.fp4_hip_gemm_small_nf4(p_(x[i:i + 16]), p_(packed), p_(absmax), None, p_(y[i:i + 16]),
                                                                      min(16, rows - i), M, K, BS, DT[dtype], s()))
                                       for i in range(0, rows, 16)])
                    cell["gemm_small_nf4_chunks_of_16"] = c
                    cell["speedup_vs_chunks_of_16"] = round(c["us"] / a["us"], 2)
                    won = won and beyond(a, c)
                d = timed(lambda: pkg.ext.gemm_small_fp4(x, B_t, absmax, BS, [M, K], None))
                cell["gemm_small_fp4_us"] = d["us"]
                cell["nf4_over_fp4"] = round(a["us"] / d["us"], 3)
                cell["gemm_wide_nf4_torch_op_us"] = timed(lambda: pkg.ext.gemm_wide_nf4(x, B_t, absmax, BS, [M, K], None))["us"]
                cell["beats_every_baseline_beyond_spread"] = won
                cells.append(cell)
        del packed, absmax
    print(json.dumps({"device": torch.cuda.get_device_name(0), "revision": args.revision, "blocksize": BS, "launches_per_graph": args.launches,
                      "reps": args.reps, "cells_won": sum(c["beats_every_baseline_beyond_spread"] for c in cells), "cells_total": len(cells),
                      "cells": cells}))


def fused_epilogues(args):
    L = lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    dev = torch.device("cuda", 0)
    s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dtype, dt = torch.bfloat16, DT[torch.bfloat16]
    qtype = pkg.ScalarType.from_torch_dtype(dtype).value

    def bind(l):
        l.fp4_hip_gemv_nf4.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp]
        for f in (l.fp4_hip_gemm_small_nf4, l.fp4_hip_gemm_wide_nf4):
            f.argtypes = [vp] * 5 + [i64] * 3 + [i32] * 2 + [vp]
        return l

    libs = {"this_tree": bind(L)}
    if args.baseline_lib:
        libs["baseline"] = bind(ctypes.CDLL(os.path.abspath(args.baseline_lib)))

    def timed(fn):
        replay = capture(lambda: [fn() for _ in range(args.launches)])
        med, samples = time_replays(replay, args.reps, args.launches)
        q = sorted(samples)
        return {"us": round(med, 2), "min_us": round(q[0], 2), "max_us": round(q[-1], 2)}

    rng_of = lambda t: t["max_us"] - t["min_us"]  # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(0)

    def nf4_weight(M, K):
        packed = torch.randint(0, 256, (M * K // 2,), dtype=torch.uint8, device=dev, generator=gen)
        absmax = torch.rand(M * K // BS, device=dev, generator=gen) * 0.02 + 0.002
        return packed, absmax

    # (1) the plain calls, this tree's library and the baseline build side by side
    plain = []
    for M, K in ((4096, 4096), (14336, 4096)):
        packed, absmax = nf4_weight(M, K)
        x = torch.randn(64, K, device=dev).to(dtype)
        y = torch.empty(64, M, dtype=dtype, device=dev)
        calls = [("gemv_nf4", 1, lambda l: l.fp4_hip_gemv_nf4(p_(x), p_(packed), p_(absmax), None, p_(y), M, K, BS, dt, s()))]
        for name, rows in (("gemm_small_nf4", 2), ("gemm_small_nf4", 16), ("gemm_wide_nf4", 32), ("gemm_wide_nf4", 64)):
            calls.append((name, rows, lambda l, name=name, rows=rows: getattr(l, "fp4_hip_" + name)(
                p_(x), p_(packed), p_(absmax), None, p_(y), rows, M, K, BS, dt, s())))
        for name, rows, fn in calls:
            cell = {"M": M, "K": K, "call": name, "rows": rows}
            for tag, l in libs.items():
                if fn(l):
                    raise RuntimeError(l.fp4_hip_last_error().decode())
                cell[tag] = timed(lambda: fn(l))
            if "baseline" in cell:
                margin = max(rng_of(cell["this_tree"]), rng_of(cell["baseline"]))
                cell["margin_us"] = round(margin, 2)
                cell["delta_us"] = round(cell["this_tree"]["us"] - cell["baseline"]["us"], 2)
                cell["within_margin"] = bool(cell["delta_us"] <= margin)
            plain.append(cell)
        del packed, absmax

    # (2) fused against the unfused sequence, Mistral-7B shapes
    H, I = 4096, 14336
    wo, wgu, wdn = nf4_weight(H, H), nf4_weight(2 * I, H), nf4_weight(H, I)
    t_ = lambda w: w[0].view(-1, 1).t()  # noqa: E731
    silu = torch.nn.functional.silu

    def lin(w, shape, x):  # the unfused op QuantData issues for this row count
        if x.shape[0] == 1:
            return pkg.ext.gemv_nf4(x, t_(w), w[1], BS, qtype, shape)
        return pkg.ext.gemm_wide_nf4(x, t_(w), w[1], BS, shape, None)

    def fused_op(w, shape, x, res, epi):
        op = pkg.ext.gemv_nf4_fused if x.shape[0] == 1 else pkg.ext.gemm_nf4_fused
        return op(x, t_(w), w[1], BS, shape, None, res, epi)

    def unfused_gate_up(h):
        g, u = lin(wgu, [2 * I, H], h).split([I, I], dim=-1)
        return silu(g) * u

    cells = []
    for rows in (1, 8, 32, 64):
        h = torch.randn(rows, H, device=dev).to(dtype)
        a = torch.randn(rows, I, device=dev).to(dtype)
        legs = {
            "o_proj_residual": (lambda: fused_op(wo, [H, H], h, h, 0), lambda: h + lin(wo, [H, H], h)),
            "gate_up_silu_mul": (lambda: fused_op(wgu, [2 * I, H], h, None, 1), lambda: unfused_gate_up(h)),
            "down_residual": (lambda: fused_op(wdn, [H, I], a, h, 0), lambda: h + lin(wdn, [H, I], a)),
            "mlp_gate_up_down_residual": (lambda: fused_op(wdn, [H, I], fused_op(wgu, [2 * I, H], h, None, 1), h, 0),
                                          lambda: h + lin(wdn, [H, I], unfused_gate_up(h))),
        }
        for leg, (f, u) in legs.items():
            tf, tu = timed(f), timed(u)
            spread = rng_of(tf) + rng_of(tu)
            cells.append({"leg": leg, "rows": rows, "fused": tf, "unfused": tu, "saved_us": round(tu["us"] - tf["us"], 2),
                          "speedup": round(tu["us"] / tf["us"], 3), "spread_us": round(spread, 2),
                          "fused_ahead_beyond_spread": bool(tu["us"] - tf["us"] > spread)})
    print(json.dumps({"device": torch.cuda.get_device_name(0), "revision": args.revision, "dtype": "bf16", "blocksize": BS,
                      "launches_per_graph": args.launches, "reps": args.reps,
                      "baseline_lib": "the parent commit's library, same run" if args.baseline_lib else "not measured",
                      "plain_calls": plain, "plain_calls_all_within_margin": (all(c["within_margin"] for c in plain) if args.baseline_lib else None),
                      "fused_vs_unfused": cells}))


def nested(args):
    L = lib()
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    dev = torch.device("cuda", 0)
    s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dtype, dt = torch.bfloat16, DT[torch.bfloat16]
    G = 256

    def bind(l):
        l.fp4_hip_gemv_nf4.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp]
        l.fp4_hip_gemm_fused_nf4.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_lora_down.argtypes = [vp, vp, vp, vp, i64, i64, i64, i32, vp]
        l.fp4_hip_gemv_lora_nf4.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemm_lora_nf4.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64, i64, i32, i32, i32, vp]
        return l

    L.fp4_hip_gemv_fused_nf4.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, vp]
    L.fp4_hip_gemv_nested_nf4.argtypes = [vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, i64, i64, i32, i32, i32, vp]
    L.fp4_hip_gemm_nested_nf4.argtypes = [vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, i64, i64, i64, i32, i32, i32, vp]
    L.fp4_hip_gemv_lora_nested_nf4.argtypes = [vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, vp, i64, vp, i64, i64, i32, i32, i32, vp]
    L.fp4_hip_gemm_lora_nested_nf4.argtypes = [vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, vp, i64, vp, i64, i64, i64, i32, i32, i32, vp]
    libs = {"this_tree": bind(L)}
    if args.baseline_lib:
        libs["baseline"] = bind(ctypes.CDLL(os.path.abspath(args.baseline_lib)))

    def timed(fn):
        replay = capture(lambda: [fn() for _ in range(args.launches)])
        med, samples = time_replays(replay, args.reps, args.launches)
        q = sorted(samples)
        return {"us": round(med, 2), "min_us": round(q[0], 2), "max_us": round(q[-1], 2)}

    def check(l, rc):
        if rc:
            raise RuntimeError(l.fp4_hip_last_error().decode())

    rng_of = lambda t: t["max_us"] - t["min_us"]  # noqa: E731
    from torch_bnb_fp4.nested import dynamic_map

    code = dynamic_map().to(dev)
    cells = []
    for M, K in SHAPES:
        n = M * K
        torch.manual_seed(0)
        w16 = (torch.randn(n, device=dev) * 0.02).to(torch.float16)
        packed = torch.empty(n // 2, dtype=torch.uint8, device=dev)
        absmax = torch.empty(n // BS, dtype=torch.float32, device=dev)
        check(L, L.fp4_hip_quantize_blockwise_nf4(p_(w16), DT[torch.float16], p_(packed), p_(absmax), n, BS, s()))
        del w16
        offset = float(absmax.mean())
        q, nabs = pkg.ext.absmax_nest(absmax, offset, code, G)
        expanded = pkg.ext.absmax_unnest(q, nabs, code, offset, G)
        x = torch.randn(K, device=dev).to(dtype)
        y = torch.empty(M, dtype=dtype, device=dev)
        y2 = torch.empty(M, dtype=dtype, device=dev)
        nested_call = lambda: check(L, L.fp4_hip_gemv_nested_nf4(p_(x), p_(packed), p_(q), p_(nabs), p_(code), offset, G, None, None, p_(y), M, K,  # noqa: E731
                                                                 BS, dt, 0, s()))
        fused_call = lambda: check(L, L.fp4_hip_gemv_fused_nf4(p_(x), p_(packed), p_(expanded), None, None, p_(y2), M, K, BS, dt, 0, s()))  # noqa: E731
        nested_call(), fused_call()
        torch.cuda.synchronize()
        cell = {"M": M, "K": K, "bit_identical": bool(torch.equal(y, y2))}
        tn, tf = timed(nested_call), timed(fused_call)
        spread = rng_of(tn) + rng_of(tf)
        delta = tn["us"] - tf["us"]
        cell.update({"gemv_nf4_nested": tn, "gemv_nf4_fused_on_expanded": tf, "delta_us": round(delta, 2), "ratio": round(tn["us"] / tf["us"], 3),
                     "spread_us": round(spread, 2), "verdict": "level" if abs(delta) <= spread else ("nested ahead" if delta < 0 else "nested behind")})
        plain = {}
        for tag, l in libs.items():
            plain[tag] = timed(lambda: check(l, l.fp4_hip_gemv_nf4(p_(x), p_(packed), p_(expanded), None, p_(y2), M, K, BS, dt, s())))
        if "baseline" in plain:
            margin = max(rng_of(plain["this_tree"]), rng_of(plain["baseline"]))
            plain.update({"margin_us": round(margin, 2), "delta_us": round(plain["this_tree"]["us"] - plain["baseline"]["us"], 2)})
            plain["within_margin"] = bool(abs(plain["delta_us"]) <= margin)
        cell["plain_gemv_nf4"] = plain
        cell["absmax_unnest"] = timed(lambda: pkg.ext.absmax_unnest(q, nabs, code, offset, G))
        for rows in (8, 64):
            xb = torch.randn(rows, K, device=dev).to(dtype)
            a = timed(lambda: pkg.ext.qlinear_nf4_nested(xb, packed, q, nabs, code, offset, G, M, K, BS, None))
            b = timed(lambda: pkg.ext.qlinear_nf4(xb, packed, expanded, M, K, BS))
            cell[f"qlinear_rows{rows}"] = {"qlinear_nf4_nested": a, "qlinear_nf4": b, "delta_us": round(a["us"] - b["us"], 2)}
        # (5) 2..64 rows: gemm_nf4_nested against the parent commit's path for the same resident layer (qlinear_nf4_nested: expand
        # into a temporary, dequant + GEMM), both as the layer issues them; then the C entry point against fp4_hip_gemm_fused_nf4 on
        # the expanded statistics, through this tree's library and the baseline's
        B_t = packed.view(-1, 1).t()
        verdict = lambda new, old: ("level" if abs(old["us"] - new["us"]) <= rng_of(new) + rng_of(old)  # noqa: E731
                                    else ("ahead" if old["us"] > new["us"] else "behind"))
        batched = []
        for rows in args.nested_rows:
            xb = torch.randn(rows, K, device=dev).to(dtype)
            yb, yb2 = torch.empty(rows, M, dtype=dtype, device=dev), torch.empty(rows, M, dtype=dtype, device=dev)
            new = lambda: pkg.ext.gemm_nf4_nested(xb, B_t, q, nabs, code, offset, G, BS, [M, K], None, None, 0)  # noqa: E731
            old = lambda: pkg.ext.qlinear_nf4_nested(xb, packed, q, nabs, code, offset, G, M, K, BS, None)  # noqa: E731
            same = bool(torch.equal(new(), pkg.ext.gemm_nf4_fused(xb, B_t, expanded, BS, [M, K], None, None, 0)))
            tn, to = timed(new), timed(old)
            c = {"rows": rows, "bit_identical_to_gemm_nf4_fused_on_expanded": same, "gemm_nf4_nested": tn, "parent_resident_path": to,
                 "saved_us": round(to["us"] - tn["us"], 2), "speedup": round(to["us"] / tn["us"], 3),
                 "spread_us": round(rng_of(tn) + rng_of(to), 2), "verdict": verdict(tn, to)}
            c["c_abi_gemm_nested_nf4"] = timed(lambda: check(L, L.fp4_hip_gemm_nested_nf4(p_(xb), p_(packed), p_(q), p_(nabs), p_(code), offset, G,
                                                                                          None, None, p_(yb), rows, M, K, BS, dt, 0, s())))
            for tag, l in libs.items():
                c[f"c_abi_gemm_fused_nf4_on_expanded_{tag}"] = timed(lambda: check(l, l.fp4_hip_gemm_fused_nf4(
                    p_(xb), p_(packed), p_(expanded), None, None, p_(yb2), rows, M, K, BS, dt, 0, s())))
            ref = c["c_abi_gemm_fused_nf4_on_expanded_" + ("baseline" if "baseline" in libs else "this_tree")]
            c["nested_vs_fused_on_expanded"] = verdict(c["c_abi_gemm_nested_nf4"], ref)
            batched.append(c)
        cell["batched"] = batched
        # (6) one rank-16 adapter: lora_down + gemv_nf4_lora_nested / gemm_nf4_lora_nested against the parent's resident path plus the
        # adapter as torch ops in the activation dtype; then the C entry points against the un-nested LoRA forms on expanded statistics
        R = 16
        A = (torch.randn(R, K, device=dev) / K ** 0.5).to(dtype)
        lB = (torch.randn(M, R, device=dev) * 0.05).to(dtype)
        sc = torch.full((R,), 2.0, device=dev)
        At, lBt, s_t = A.t().contiguous(), lB.t().contiguous(), sc.to(dtype)
        with_adapter = []
        for rows in args.nested_lora_rows:
            xb = torch.randn(rows, K, device=dev).to(dtype)
            yb, yb2, tb = torch.empty(rows, M, dtype=dtype, device=dev), torch.empty(rows, M, dtype=dtype, device=dev), torch.empty(rows, R, device=dev)
            if rows == 1:
                new = lambda: pkg.ext.gemv_nf4_lora_nested(xb, B_t, q, nabs, code, offset, G, BS, [M, K], None, None, 0, lB,  # noqa: E731
                                                           pkg.ext.lora_down(xb, A, sc))
                old = lambda: pkg.ext.gemv_nf4_nested(xb, B_t, q, nabs, code, offset, G, BS, [M, K], None, None, 0) + ((xb @ At) * s_t) @ lBt  # noqa: E731
                ref_op = lambda: pkg.ext.gemv_nf4_lora(xb, B_t, expanded, BS, [M, K], None, None, 0, lB, pkg.ext.lora_down(xb, A, sc))  # noqa: E731
                c_new = lambda l: (check(l, l.fp4_hip_lora_down(p_(xb), p_(A), p_(sc), p_(tb), rows, R, K, dt, s())),  # noqa: E731
                                   check(l, l.fp4_hip_gemv_lora_nested_nf4(p_(xb), p_(packed), p_(q), p_(nabs), p_(code), offset, G, None, None, p_(lB),
                                                                           p_(tb), R, p_(yb), M, K, BS, dt, 0, s())))
                c_ref = lambda l: (check(l, l.fp4_hip_lora_down(p_(xb), p_(A), p_(sc), p_(tb), rows, R, K, dt, s())),  # noqa: E731
                                   check(l, l.fp4_hip_gemv_lora_nf4(p_(xb), p_(packed), p_(expanded), None, None, p_(lB), p_(tb), R, p_(yb2), M, K, BS,
                                                                    dt, 0, s())))
            else:
                new = lambda: pkg.ext.gemm_nf4_lora_nested(xb, B_t, q, nabs, code, offset, G, BS, [M, K], None, None, 0, lB,  # noqa: E731
                                                           pkg.ext.lora_down(xb, A, sc))
                old = lambda: pkg.ext.qlinear_nf4_nested(xb, packed, q, nabs, code, offset, G, M, K, BS, None) + ((xb @ At) * s_t) @ lBt  # noqa: E731
                ref_op = lambda: pkg.ext.gemm_nf4_lora(xb, B_t, expanded, BS, [M, K], None, None, 0, lB, pkg.ext.lora_down(xb, A, sc))  # noqa: E731
                c_new = lambda l: (check(l, l.fp4_hip_lora_down(p_(xb), p_(A), p_(sc), p_(tb), rows, R, K, dt, s())),  # noqa: E731
                                   check(l, l.fp4_hip_gemm_lora_nested_nf4(p_(xb), p_(packed), p_(q), p_(nabs), p_(code), offset, G, None, None, p_(lB),
                                                                           p_(tb), R, p_(yb), rows, M, K, BS, dt, 0, s())))
                c_ref = lambda l: (check(l, l.fp4_hip_lora_down(p_(xb), p_(A), p_(sc), p_(tb), rows, R, K, dt, s())),  # noqa: E731
                                   check(l, l.fp4_hip_gemm_lora_nf4(p_(xb), p_(packed), p_(expanded), None, None, p_(lB), p_(tb), R, p_(yb2), rows, M, K,
                                                                    BS, dt, 0, s())))
            same = bool(torch.equal(new(), ref_op()))
            tn, to = timed(new), timed(old)
            c = {"rows": rows, "rank": R, "bit_identical_to_the_lora_op_on_expanded": same, "lora_down_plus_nested_lora_op": tn,
                 "parent_resident_path_plus_torch_adapter": to, "saved_us": round(to["us"] - tn["us"], 2), "speedup": round(to["us"] / tn["us"], 3),
                 "spread_us": round(rng_of(tn) + rng_of(to), 2), "verdict": verdict(tn, to),
                 "lora_fused_ahead": bool(pkg.fused.lora_fused_ahead(rows, M, K, R))}
            c["c_abi_nested_pair"] = timed(lambda: c_new(L))
            for tag, l in libs.items():
                c[f"c_abi_lora_pair_on_expanded_{tag}"] = timed(lambda: c_ref(l))
            ref = c["c_abi_lora_pair_on_expanded_" + ("baseline" if "baseline" in libs else "this_tree")]
            c["nested_vs_lora_on_expanded"] = verdict(c["c_abi_nested_pair"], ref)
            with_adapter.append(c)
        cell["rank16_adapter"] = with_adapter
        resident = q.numel() + 4 * nabs.numel() + 4 * code.numel()
        cell["statistics_bytes"] = {"resident": resident, "expanded": 4 * expanded.numel(), "packed_weight": packed.numel(),
                                    "bits_per_weight_resident": round(8 * resident / n, 4), "bits_per_weight_expanded": round(32 * expanded.numel() / n, 4)}
        cells.append(cell)
        del packed, absmax, q, nabs, expanded
    print(json.dumps({"device": torch.cuda.get_device_name(0), "revision": args.revision, "dtype": "bf16", "blocksize": BS, "nested_blocksize": G,
                      "launches_per_graph": args.launches, "reps": args.reps,
                      "baseline_lib": "the parent commit's library, same run" if args.baseline_lib else "not measured",
                      "plain_gemv_all_within_margin": (all(c["plain_gemv_nf4"]["within_margin"] for c in cells) if args.baseline_lib else None),
                      "all_bit_identical": all(c["bit_identical"] and all(b["bit_identical_to_gemm_nf4_fused_on_expanded"] for b in c["batched"])
                                               and all(a["bit_identical_to_the_lora_op_on_expanded"] for a in c["rank16_adapter"]) for c in cells),
                      "batched_cells_ahead_of_the_parent_resident_path": sum(b["verdict"] == "ahead" for c in cells for b in c["batched"]),
                      "batched_cells_total": sum(len(c["batched"]) for c in cells),
                      "adapter_cells_ahead_of_the_parent_resident_path": sum(a["verdict"] == "ahead" for c in cells for a in c["rank16_adapter"]),
                      "adapter_cells_total": sum(len(c["rank16_adapter"]) for c in cells), "cells": cells}))


def lora(args):
    dev = torch.device("cuda", 0)
    silu = torch.nn.functional.silu

    def timed(fn):
        replay = capture(lambda: [fn() for _ in range(args.launches)])
        med, samples = time_replays(replay, args.reps, args.launches)
        q = sorted(samples)
        return {"us": round(med, 2), "min_us": round(q[0], 2), "max_us": round(q[-1], 2)}

    rng_of = lambda t: t["max_us"] - t["min_us"]  # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(0)
    cells = []
    for M, K in SHAPES:
        packed = torch.randint(0, 256, (M * K // 2,), dtype=torch.uint8, device=dev, generator=gen)
        absmax = torch.rand(M * K // BS, device=dev, generator=gen) * 0.02 + 0.002
        B_t = packed.view(-1, 1).t()
        epi = 1 if M == 28672 else 0  # the gate|up weight of the decoder
        for dtype in (torch.bfloat16, torch.float16):
            for R in args.lora_ranks:
                A = (torch.randn(R, K, device=dev, generator=gen) / K ** 0.5).to(dtype)
                lB = (torch.randn(M, R, device=dev, generator=gen) * 0.05).to(dtype)
                sc = torch.full((R,), 2.0, device=dev)
                At, lBt, s_t = A.t().contiguous(), lB.t().contiguous(), sc.to(dtype)
                for rows in args.lora_rows:
                    x = torch.randn(rows, K, device=dev, generator=gen).to(dtype)
                    base_op = pkg.ext.gemv_nf4_fused if rows == 1 else pkg.ext.gemm_nf4_fused
                    lora_op = pkg.ext.gemv_nf4_lora if rows == 1 else pkg.ext.gemm_nf4_lora
                    fused = lambda: lora_op(x, B_t, absmax, BS, [M, K], None, None, epi, lB, pkg.ext.lora_down(x, A, sc))  # noqa: E731
                    free = lambda: base_op(x, B_t, absmax, BS, [M, K], None, None, epi)  # noqa: E731
                    if epi:
                        def unfused():
                            y = base_op(x, B_t, absmax, BS, [M, K], None, None, 0) + ((x @ At) * s_t) @ lBt
                            return silu(y[..., 0::2]) * y[..., 1::2]
                    else:
                        unfused = lambda: base_op(x, B_t, absmax, BS, [M, K], None, None, 0) + ((x @ At) * s_t) @ lBt  # noqa: E731
                    ta, tb, tc = timed(fused), timed(unfused), timed(free)
                    spread = rng_of(ta) + rng_of(tb)
                    cells.append({"M": M, "K": K, "epilogue": "silu_mul" if epi else "none", "dtype": NAME[dtype], "rank": R, "rows": rows,
                                  "fused_down_plus_lora_op": ta, "fused_nf4_op_plus_torch_adapter": tb, "fused_nf4_op_alone": tc,
                                  "adapter_cost_us": round(ta["us"] - tc["us"], 2), "saved_us": round(tb["us"] - ta["us"], 2),
                                  "speedup": round(tb["us"] / ta["us"], 3), "spread_us": round(spread, 2),
                                  "fused_ahead_beyond_spread": bool(tb["us"] - ta["us"] > spread)})
        del packed, absmax
    print(json.dumps({"device": torch.cuda.get_device_name(0), "revision": args.revision, "blocksize": BS, "launches_per_graph": args.launches,
                      "reps": args.reps, "cells_won": sum(c["fused_ahead_beyond_spread"] for c in cells), "cells_total": len(cells),
                      "cells": cells}))


def multi_lora(args):
    from torch_bnb_fp4 import fused

    dev = torch.device("cuda", 0)
    dtype, dt = torch.bfloat16, DT[torch.bfloat16]
    N_STACK = 8
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def timed(fn):
        replay = capture(lambda: [fn() for _ in range(args.launches)])
        med, samples = time_replays(replay, args.reps, args.launches)
        q = sorted(samples)
        return {"us": round(med, 2), "min_us": round(q[0], 2), "max_us": round(q[-1], 2)}

    def bind(l):
        l.fp4_hip_gemv_fused_nf4.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemm_fused_nf4.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_lora_down.argtypes = [vp, vp, vp, vp, i64, i64, i64, i32, vp]
        l.fp4_hip_gemm_lora_nf4.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64, i64, i32, i32, i32, vp]
        return l

    libs = {"this_tree": bind(ctypes.CDLL(pkg.HIP_LIBRARY_PATH))}
    if args.baseline_lib:
        libs["baseline"] = bind(ctypes.CDLL(os.path.abspath(args.baseline_lib)))
    rng_of = lambda t: t["max_us"] - t["min_us"]  # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(0)
    cells, unchanged = [], []
    for M, K in SHAPES:
        packed = torch.randint(0, 256, (M * K // 2,), dtype=torch.uint8, device=dev, generator=gen)
        absmax = torch.rand(M * K // BS, device=dev, generator=gen) * 0.02 + 0.002
        B_t = packed.view(-1, 1).t()
        epi = 1 if M == 28672 else 0  # the gate|up weight of the decoder
        base = fused.FusedNF4Linear(fused.FusedNF4Linear.from_packed(packed.view(-1, 1), absmax, (M, K), BS, dtype=dtype).quant_data, epi)
        Mo = M // 2 if epi else M
        if args.baseline_lib:  # the entry points that existed before, through both libraries: ISA-identical, so within the ranges
            x1, x32 = (torch.randn(r, K, device=dev, generator=gen).to(dtype) for r in (1, 32))
            A16 = (torch.randn(16, K, device=dev, generator=gen) / K ** 0.5).to(dtype)
            B16 = (torch.randn(M, 16, device=dev, generator=gen) * 0.05).to(dtype)
            sc16, t32 = torch.full((16,), 2.0, device=dev), torch.zeros(32, 16, device=dev)
            y1, y32 = torch.empty(1, Mo, dtype=dtype, device=dev), torch.empty(32, Mo, dtype=dtype, device=dev)
            calls = {
                "gemv_fused_nf4": lambda l: l.fp4_hip_gemv_fused_nf4(p_(x1), p_(packed), p_(absmax), None, None, p_(y1), M, K, BS, dt, epi, s()),
                "gemm_fused_nf4_32": lambda l: l.fp4_hip_gemm_fused_nf4(p_(x32), p_(packed), p_(absmax), None, None, p_(y32), 32, M, K, BS, dt, epi, s()),
                "lora_down_32": lambda l: l.fp4_hip_lora_down(p_(x32), p_(A16), p_(sc16), p_(t32), 32, 16, K, dt, s()),
                "gemm_lora_nf4_32": lambda l: l.fp4_hip_gemm_lora_nf4(p_(x32), p_(packed), p_(absmax), None, None, p_(B16), p_(t32), 16, p_(y32), 32,
                                                                      M, K, BS, dt, epi, s()),
            }
            for name, call in calls.items():
                both = {tag: timed(lambda: call(l)) for tag, l in libs.items()}
                margin = max(rng_of(both["this_tree"]), rng_of(both["baseline"]))
                delta = both["this_tree"]["us"] - both["baseline"]["us"]
                unchanged.append({"M": M, "K": K, "entry": name, **both, "delta_us": round(delta, 2), "margin_us": round(margin, 2),
                                  "within_margin": bool(abs(delta) <= margin)})
        for R in args.lora_ranks:
            A_stack = (torch.randn(N_STACK, R, K, device=dev, generator=gen) / K ** 0.5).to(dtype)
            B_stack = (torch.randn(N_STACK, M, R, device=dev, generator=gen) * 0.05).to(dtype)
            s_stack = torch.full((N_STACK, R), 2.0, device=dev)
            singles = [fused.LoRANF4Linear.from_fused(base, A_stack[a], B_stack[a], s_stack[a]) for a in range(N_STACK)]
            print(f"multi-lora: {M}x{K} rank {R}", file=sys.stderr, flush=True)
            for rows in args.lora_rows:
                if rows < 2:
                    continue
                x = torch.randn(rows, K, device=dev, generator=gen).to(dtype)
                for distinct in (1, 4, 8):
                    for order in (("sorted",) if distinct == 1 else ("sorted", "interleaved")):
                        ids = [b * distinct // rows for b in range(rows)] if order == "sorted" else [b % distinct for b in range(rows)]
                        idt = torch.tensor(ids, dtype=torch.int32, device=dev)
                        groups = [torch.tensor([b for b in range(rows) if ids[b] == a], dtype=torch.int64, device=dev) for a in range(distinct)]

                        def multi():
                            t = pkg.ext.lora_down_multi(x, A_stack, s_stack, idt)
                            return pkg.ext.gemm_nf4_lora_multi(x, B_t, absmax, BS, [M, K], None, None, epi, B_stack, idt, t)

                        def grouped():
                            if distinct == 1:  # the single-adapter fused pair, as LoRANF4Linear issues it where it is ahead
                                return pkg.ext.gemm_nf4_lora(x, B_t, absmax, BS, [M, K], None, None, epi, B_stack[0], pkg.ext.lora_down(x, A_stack[0], s_stack[0]))
                            out = torch.empty(rows, Mo, dtype=dtype, device=dev)
                            for a, idx in enumerate(groups):
                                out.index_copy_(0, idx, singles[a](x.index_select(0, idx)))
                            return out

                        same = bool(torch.equal(multi(), grouped()))
                        ta, tb = timed(multi), timed(grouped)
                        spread = rng_of(ta) + rng_of(tb)
                        delta = tb["us"] - ta["us"]
                        cells.append({"M": M, "K": K, "epilogue": "silu_mul" if epi else "none", "rank": R, "rows": rows, "distinct_adapters": distinct,
                                      "ids": order, "lora_fused_ahead": bool(fused.lora_fused_ahead(rows, M, K, R)),
                                      "fused_multi": ta, "baseline": tb,
                                      "baseline_is": "single-adapter fused pair" if distinct == 1 else "grouped index_select / LoRANF4Linear / index_copy",
                                      "same_values_as_baseline": same, "saved_us": round(delta, 2), "speedup": round(tb["us"] / ta["us"], 3),
                                      "spread_us": round(spread, 2),
                                      "verdict": "level" if abs(delta) <= spread else ("ahead" if delta > 0 else "behind")})
            del A_stack, B_stack, singles
        del packed, absmax, base
    inside = [c for c in cells if c["lora_fused_ahead"] and c["distinct_adapters"] > 1]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "revision": args.revision, "dtype": "bf16", "blocksize": BS, "adapters_in_stack": N_STACK,
                      "launches_per_graph": args.launches, "reps": args.reps,
                      "baseline_lib": "the parent commit's library, same run" if args.baseline_lib else "not measured",
                      "pre_existing_entry_points_all_within_margin": (all(u["within_margin"] for u in unchanged) if unchanged else None),
                      "mixed_cells_inside_lora_fused_ahead": len(inside), "of_which_ahead": sum(c["verdict"] == "ahead" for c in inside),
                      "of_which_level": sum(c["verdict"] == "level" for c in inside), "of_which_behind": sum(c["verdict"] == "behind" for c in inside),
                      "pre_existing_entry_points": unchanged, "cells": cells}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--small-batch", action="store_true", help="the 2..16-row NF4 regime (profiles/nf4_small_batch.json)")
    ap.add_argument("--wide-batch", action="store_true", help="the 17..128-row NF4 regime (profiles/nf4_wide_batch.json)")
    ap.add_argument("--revision", default="unknown", help="--wide-batch: the git revision the figures belong to, recorded as given")
    ap.add_argument("--fused", action="store_true", help="the fused NF4 decode epilogues (profiles/nf4_fused_epilogues.json)")
    ap.add_argument("--baseline-lib", default=None, help="--fused / --nested: another build of libtorch_bnb_fp4_hip.so to time the plain calls of, side by side")
    ap.add_argument("--lora", action="store_true", help="LoRA adapters beside NF4 weights, fused against torch ops (profiles/nf4_lora.json)")
    ints = lambda v: [int(i) for i in v.split(",")]  # noqa: E731
    ap.add_argument("--lora-ranks", type=ints, default=[16, 64], help="--lora: adapter ranks (multiples of 8), comma-separated")
    ap.add_argument("--lora-rows", type=ints, default=[1, 8, 32, 64], help="--lora: activation row counts (1..64), comma-separated")
    ap.add_argument("--multi-lora", action="store_true",
                    help="several adapters per batch, fused multi-adapter ops against rows grouped by adapter (profiles/nf4_multi_lora.json)")
    ap.add_argument("--nested", action="store_true", help="double-quantised absmax: the nested GEMV, unnest and qlinear_nf4_nested (profiles/nf4_nested.json)")
    ap.add_argument("--nested-rows", type=ints, default=[2, 8, 16, 32, 64], help="--nested: row counts of the batched cells, comma-separated")
    ap.add_argument("--nested-lora-rows", type=ints, default=[1, 8, 32], help="--nested: row counts of the rank-16 adapter cells, comma-separated")
    args = ap.parse_args()
    if args.nested:
        return nested(args)
    if args.multi_lora:
        if args.lora_rows == [1, 8, 32, 64]:
            args.lora_rows = [8, 32, 64]
        return multi_lora(args)
    if args.lora:
        return lora(args)
    if args.fused:
        return fused_epilogues(args)
    if args.small_batch:
        return small_batch(args)
    if args.wide_batch:
        return wide_batch(args)
    L = lib()
    dev = torch.device("cuda", 0)
    s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def check(rc):
        if rc:
            raise RuntimeError(L.fp4_hip_last_error().decode())

    def us(fn):
        replay = capture(lambda: [fn() for _ in range(args.launches)])
        return round(time_replays(replay, args.reps, args.launches)[0], 2)

    rows = []
    for M, K in SHAPES:
        n = M * K
        torch.manual_seed(0)
        w16 = (torch.randn(n, device=dev) * 0.02).to(torch.float16)
        pk = {}
        for qt, fn in (("fp4", L.fp4_hip_quantize_blockwise), ("nf4", L.fp4_hip_quantize_blockwise_nf4)):
            packed = torch.empty(n // 2, dtype=torch.uint8, device=dev)
            absmax = torch.empty(n // BS, dtype=torch.float32, device=dev)
            check(fn(p_(w16), DT[torch.float16], p_(packed), p_(absmax), n, BS, s()))
            pk[qt] = (packed, absmax)
        del w16
        for dtype in (torch.bfloat16, torch.float16, torch.float32):
            r = {"M": M, "K": K, "dtype": NAME[dtype]}
            out = torch.empty(n, dtype=dtype, device=dev)
            x = torch.randn(K, device=dev).to(dtype)
            y = torch.empty(M, dtype=dtype, device=dev)
            for qt, table in (("fp4", TREE), ("nf4", NF4)):
                packed, absmax = pk[qt]
                r[f"dequant_{qt}_us"] = us(lambda: check(L.fp4_hip_dequantize_blockwise(p_(packed), p_(absmax), p_(out), BS, n, DT[dtype], table, 0, s())))
                g = L.fp4_hip_gemv if qt == "fp4" else L.fp4_hip_gemv_nf4
                r[f"gemv_{qt}_us"] = us(lambda: check(g(p_(x), p_(packed), p_(absmax), None, p_(y), M, K, BS, DT[dtype], s())))
            del out
            packed, absmax = pk["nf4"]
            x2 = x.view(1, K)
            r["nf4_dequant_hipblaslt_batch1_us"] = us(lambda: pkg.ext.qlinear_nf4(x2, packed, absmax, M, K, BS))
            r["gemv_nf4_over_fp4"] = round(r["gemv_nf4_us"] / r["gemv_fp4_us"], 3)
            r["dequant_nf4_over_fp4"] = round(r["dequant_nf4_us"] / r["dequant_fp4_us"], 3)
            r["gemv_nf4_speedup_vs_dequant_gemm"] = round(r["nf4_dequant_hipblaslt_batch1_us"] / r["gemv_nf4_us"], 2)
            if dtype == torch.bfloat16:  # LDS-table layout ablation of the NF4 GEMV
                for v in (0, 1):
                    L.fp4_hip_set_variant(b"gemv_nf4", v)
                    r[f"gemv_nf4_table{v}_us"] = us(lambda: check(L.fp4_hip_gemv_nf4(p_(x), p_(packed), p_(absmax), None, p_(y), M, K, BS, DT[dtype], s())))
                L.fp4_hip_set_variant(b"gemv_nf4", -1)
            w = (torch.randn(n, device=dev) * 0.02).to(dtype)
            qp = torch.empty(n // 2, dtype=torch.uint8, device=dev)
            qa = torch.empty(n // BS, dtype=torch.float32, device=dev)
            for qt, fn in (("fp4", L.fp4_hip_quantize_blockwise), ("nf4", L.fp4_hip_quantize_blockwise_nf4)):
                r[f"quantize_{qt}_us"] = us(lambda: check(fn(p_(w), DT[dtype], p_(qp), p_(qa), n, BS, s())))
            r["quantize_nf4_over_fp4"] = round(r["quantize_nf4_us"] / r["quantize_fp4_us"], 3)
            del w, qp, qa
            rows.append(r)
        del pk

    # steady state: one launch per weight over a stack of distinct tall weights (~1.9 GB of NF4 bytes, far beyond the caches)
    M, K, depth = 28672, 4096, 32
    stack = [torch.randint(0, 256, (M * K // 2,), dtype=torch.uint8, device=dev) for _ in range(depth)]
    scales = [torch.rand(M * K // BS, device=dev) for _ in range(depth)]
    x = torch.randn(K, device=dev).to(torch.bfloat16)
    y = torch.empty(M, dtype=torch.bfloat16, device=dev)
    replay = capture(lambda: [check(L.fp4_hip_gemv_nf4(p_(x), p_(pk_), p_(am), None, p_(y), M, K, BS, 2, s())) for pk_, am in zip(stack, scales)])
    per = time_replays(replay, args.reps, depth)[0]
    bytes_per = M * K // 2 + M * K // BS * 4 + K * 2 + M * 2
    steady = {"M": M, "K": K, "dtype": "bf16", "weights": depth, "us_per_weight": round(per, 2),
              "TBps": round(bytes_per / (per * 1e-6) / 1e12, 2), "fraction_of_8TBps": round(bytes_per / (per * 1e-6) / SPEC_BPS, 3)}
    print(json.dumps({"device": torch.cuda.get_device_name(0), "blocksize": BS, "launches_per_graph": args.launches, "reps": args.reps,
                      "rows": rows, "gemv_nf4_steady_state": steady}))


if __name__ == "__main__":
    main()
