#!/usr/bin/env python3
"""The biased attention core (shl_mi355x_attention_bias) against the launches it replaces, through the C-ABI (no torch).

    python tools/attention_bias_bench.py [--reps 4] [--windows 7] [--window-ms 40] [--only NAME[,NAME]] [--dtypes int8,f16] [--lib DIR] [--out FILE.md]
Per shape and dtype four hipGraphs are captured, each holding `reps` units of work that rotate over three buffer sets (so that
a unit does not find its operands in the last-level cache):
  * fused      one launch per unit: what a session's STEP_ATTENTION enqueues for a chain with the add;
  * unfused    the five launches the same session captures with SHL_MI355X_ATTENTION=0: shl_mi355x_matmul (q k^T),
               shl_mi355x_mul, shl_mi355x_add_bcast, shl_mi355x_softmax, shl_mi355x_matmul (p v) -- kernels this change leaves
               as they were -- with the scores three times and the probabilities once through HBM;
  * the same pair without the add (shl_mi355x_attention against its four launches), as the yardstick: the biased launch
    removes one launch and one round trip more, so its ratio should be no worse than the unbiased one's.
A window is as many replays of one graph between two HIP events as last --window-ms (40 ms; 20 at the least).  The windows of
a pair ALTERNATE (unfused, fused, unfused, ...), so that a drift of the clocks falls on both sides alike; the figure is the
median window per unit, "spread" the range of a side's windows over its median.  "admit": the fused median is below the unfused one by more than the spread (in time) of either
side -- the condition csrc/attention_canon.h:att_bias_default's classes have to meet.  Before timing, the fused output is
compared with the unfused one bit for bit.  --lib DIR times the native libraries of another build (an A/B of two kernels).

Shapes (images x heads, S, T, d; bias): a DETR encoder layer (8 heads, 850 tokens, d 32; padding mask [B,1,1,T]), a Swin-T
stage-1 block (64 windows an image, 3 heads, 49 tokens, d 32; relative position bias [1,3,49,49]), BERT-base (12 heads, 128
and 384 tokens, d 64; padding mask), ViT-B/16 (12 heads, 197 tokens, d 64; a relative position bias [1,12,197,197]), each at
batch 1 and 8.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETS = 3
SHAPES = [
    # name, images (or windows), heads, S, T, d, bias kind: "mask" [B,1,1,T] / "rel" [1,H,S,T]
    ("detr_enc_b1", 1, 8, 850, 850, 32, "mask"),
    ("detr_enc_b8", 8, 8, 850, 850, 32, "mask"),
    ("swin_t_s1_b1", 64, 3, 49, 49, 32, "rel"),
    ("swin_t_s1_b8", 512, 3, 49, 49, 32, "rel"),
    ("bert_base_128_b1", 1, 12, 128, 128, 64, "mask"),
    ("bert_base_128_b8", 8, 12, 128, 128, 64, "mask"),
    ("bert_base_384_b1", 1, 12, 384, 384, 64, "mask"),
    ("bert_base_384_b8", 8, 12, 384, 384, 64, "mask"),
    ("vit_b16_b1", 1, 12, 197, 197, 64, "rel"),
    ("vit_b16_b8", 8, 12, 197, 197, 64, "rel"),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--only", default="")
    ap.add_argument("--dtypes", default="int8,f16")
    ap.add_argument("--lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import attention_cases as ac
    import cases
    import eltwise_cases
    from pool_cases import _q
    pkg = cases.pkg
    if a.lib:
        pkg.LIB_DIR = os.path.abspath(a.lib)
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("attention_bias_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
    pkg.check(hip.shl_mi355x_set_device(0), hip, "set_device")
    dev = cases.HipDevice(hip)
    stream = hip.shl_mi355x_stream_create()
    ev0, ev1 = hip.shl_mi355x_event_create(), hip.shl_mi355x_event_create()
    ms = C.c_float()

    def capture(enqueue, reps):
        enqueue(0)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "warm-up")
        pkg.check(hip.shl_mi355x_graph_begin(stream), hip, "graph_begin")
        for k in range(reps):
            enqueue(k)
        g = hip.shl_mi355x_graph_end(stream)
        if not g:
            raise SystemExit("attention_bias_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
        hip.shl_mi355x_graph_launch(g, stream)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "first replay")
        return g

    def window(g, replays):
        hip.shl_mi355x_event_record(ev0, stream)
        for _ in range(replays):
            hip.shl_mi355x_graph_launch(g, stream)
        hip.shl_mi355x_event_record(ev1, stream)
        pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "timed window")
        hip.shl_mi355x_event_elapsed_ms(ev0, ev1, C.byref(ms))
        return ms.value

    def alternate(first, second, reps):
        """(median, range) in seconds per unit of each of two graphs whose windows alternate"""
        ga, gb = capture(first, reps), capture(second, reps)
        # as many replays as make a window of the slower graph last a.window_ms: a shorter one times the clock and the scheduler
        replays = max(20, int(np.ceil(20 * a.window_ms / max(window(ga, 20), window(gb, 20)))))
        wa, wb = [], []
        for _ in range(a.windows):
            wa.append(window(ga, replays))
            wb.append(window(gb, replays))
        hip.shl_mi355x_graph_destroy(ga)
        hip.shl_mi355x_graph_destroy(gb)
        per = 1e-3 / (replays * reps)
        return [(float(np.median(w)) * per, (max(w) - min(w)) * per) for w in (wa, wb)]

    head = ["shape", "images x heads x S x T x d", "bias", "dtype", "unfused (5) us", "spread", "fused us", "spread", "fused / unfused", "admit",
            "no bias: fused / unfused (4)"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    only = set(filter(None, a.only.split(",")))
    for name, images, heads, s, t, d, kind in SHAPES:
        if only and name not in only:
            continue
        for dtype in a.dtypes.split(","):
            batches = images * heads
            made = []
            ac._add(made, name, dtype, s=s, t=t, d=d, dv=d, batches=batches, regime="conv")
            c = made[0]
            rng = ac._rng("attention bias bench " + c["name"])
            shape = (images, 1, 1, t) if kind == "mask" else (1, heads, s, t)
            if dtype == "int8":
                xs, xz = c["sc_q"]
                if kind == "mask":  # -128 saturates the sum
                    c["bias"], c["b_q"], c["sb_q"] = np.where(rng.random(shape) < 0.2, -128, 0).astype(np.int8), _q(xs * 4.0, 0), _q(xs, xz)
                else:
                    c["bias"], c["b_q"], c["sb_q"] = rng.integers(-128, 128, shape, dtype=np.int8), _q(xs * 0.43, 3), _q(xs * 1.31, -5)
            else:
                c["bias"] = (np.where(rng.random(shape) < 0.2, -np.inf, 0.0) if kind == "mask" else rng.integers(-16, 17, shape) / 16.0).astype(np.float16)
                c["b_q"] = c["sb_q"] = _q(1.0, 0)
            es = c["q"].itemsize
            code = pkg.SHL_I8 if dtype == "int8" else pkg.SHL_F16
            bufs = []
            for _ in range(SETS):
                b = {key: dev.alloc(c[key].nbytes) for key in ("q", "k", "v", "c", "bias")}
                for key in ("q", "k", "v", "c", "bias"):
                    dev.upload(b[key], c[key])
                for key in ("s", "x", "sum", "p"):
                    b[key] = dev.alloc(batches * s * t * es)
                for key in ("chain", "fused"):
                    b[key] = dev.alloc(batches * s * d * es)
                bufs.append(b)
            desc = ac.desc(c)
            qk, mul, pv = ac.unfused_descs(c)
            add = eltwise_cases.mul_desc(dict(dtype=dtype, in_q=c["sc_q"], in1_q=c["b_q"], out_q=c["sb_q"]), (images, heads, s, t), shape)
            bd = pkg.AttentionBiasDesc()
            pkg.check(hip.shl_mi355x_attention_bias_geometry(C.byref(add), batches, s, t, C.byref(bd)), hip, "attention_bias_geometry")
            (bd.b_scale, bd.b_zp), (bd.sb_scale, bd.sb_zp) = c["b_q"], c["sb_q"]

            def unfused(kk, bias=True):
                b = bufs[kk % SETS]
                pkg.check(hip.shl_mi355x_matmul(b["q"], b["k"], b["s"], C.byref(qk), stream), hip, "matmul (q k^T)")
                pkg.check(hip.shl_mi355x_mul(b["s"], b["c"], b["x"], C.byref(mul), stream), hip, "mul")
                x, x_q = b["x"], c["sc_q"]
                if bias:
                    pkg.check(hip.shl_mi355x_add_bcast(b["x"], b["bias"], b["sum"], C.byref(add), stream), hip, "add_bcast")
                    x, x_q = b["sum"], c["sb_q"]
                pkg.check(hip.shl_mi355x_softmax(x, b["p"], code, batches * s, t, 1, x_q[0], x_q[1], c["p_q"][0], c["p_q"][1], stream), hip,
                          "softmax")
                pkg.check(hip.shl_mi355x_matmul(b["p"], b["v"], b["chain"], C.byref(pv), stream), hip, "matmul (p v)")

            def fused(kk, bias=True):
                b = bufs[kk % SETS]
                if bias:
                    pkg.check(hip.shl_mi355x_attention_bias(b["q"], b["k"], b["v"], b["bias"], b["fused"], C.byref(desc), C.byref(bd), stream),
                              hip, "attention_bias")
                else:
                    pkg.check(hip.shl_mi355x_attention(b["q"], b["k"], b["v"], b["fused"], C.byref(desc), stream), hip, "attention")

            def fetch(p):
                pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                return dev.download(p, (batches * s * d,), c["q"].dtype).view(np.uint8 if es == 1 else np.uint16)
            b0 = bufs[0]
            cells = [name, "%d x %d x %d x %d x %d" % (images, heads, s, t, d), "[B,1,1,T]" if kind == "mask" else "[1,H,S,T]", dtype]
            if hip.shl_mi355x_attention_bias_kernel_name(b0["q"], b0["k"], b0["v"], b0["bias"], b0["fused"], C.byref(desc), C.byref(bd)) == b"":
                cells += ["-", "-", "no kernel: " + hip.shl_mi355x_last_error().decode(), "-", "-", "-", "-"]
            else:
                unfused(0)
                want = fetch(b0["chain"])
                fused(0)
                if not np.array_equal(fetch(b0["fused"]), want):
                    raise SystemExit("attention_bias_bench: %s %s: the fused launch differs from the unfused launches" % (name, dtype))
                (t_un, r_un), (t_f, r_f) = alternate(unfused, fused, a.reps)
                (p_un, _), (p_f, _) = alternate(lambda kk: unfused(kk, False), lambda kk: fused(kk, False), a.reps)
                admit = t_f < t_un and (t_un - t_f) > max(r_un, r_f)
                cells += ["%.2f" % (t_un * 1e6), "%.0f %%" % (100 * r_un / t_un), "%.2f" % (t_f * 1e6), "%.0f %%" % (100 * r_f / t_f),
                          "%.2f" % (t_f / t_un), "yes" if admit else "no", "%.2f" % (p_f / p_un)]
            row = "| " + " | ".join(cells) + " |"
            lines.append(row)
            print(row, flush=True)
            for b in bufs:
                for p in b.values():
                    dev.free(p)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
