#!/usr/bin/env python3
"""One layout launch (shl_mi355x_attention_layout) against what an attention block costs without it, through the C-ABI (no torch).

    python tools/attention_layout_bench.py [--reps 4] [--windows 7] [--window-ms 40] [--only NAME[,NAME]] [--dtypes int8,f16] [--lib DIR] [--out FILE.md]
The block is a model's: q, k and v arrive as [B, S, H d], each goes through a reshape and a transpose(0,2,1,3), the core runs on
[B H][S][d], a transpose(0,2,1,3) and a reshape merge the heads again.  Per shape and dtype three hipGraphs are captured, each
holding `reps` units of work that rotate over three buffer sets (so that a unit does not find its operands in the last-level
cache):
  * A        the eight mover launches (shl_mi355x_move, shl_mi355x_transpose) around the core as a session WITHOUT the layout form
             runs it by its own default rules: one fused launch where shl_mi355x_attention[_bias]_by_default says so, else the
             four or five launches (matmul, mul, [add_bcast], softmax, matmul);
  * A'       the same movers around the other choice of core, for reference;
  * B        one layout launch.
A window is as many replays of one graph between two HIP events as last --window-ms (40 ms; 20 at the least).  The windows of a
pair ALTERNATE (A, B, A, ...), so that a drift of the clocks falls on both sides alike; the figure is the median window per
unit, "spread" the range of a side's windows, in microseconds per unit.  "admit": B's median is below A's by more than the spread (in
time) of either side -- the condition csrc/attention_canon.h:att_layout_default's classes have to meet, in both dtypes.  Before
timing, B's output is compared with A's bit for bit.  --lib DIR times the native libraries of another build.

Shapes (images, heads, S, T, d; bias): the rows of profiles/attention_notes.md and attention_bias_notes.md -- ViT-B/16 and
DeiT-tiny at batch 1 and 8, MobileViT's 64 tokens, encoders of 384, 512 and 640 tokens, a DETR encoder layer (850 tokens, d 32),
Swin-T stage-1 windows (49 keys, d 32, a relative position bias), BERT-base on 128 tokens with a padding mask.
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
    # name, images (or windows), heads, S, T, d, bias kind: None / "mask" [B,1,1,T] / "rel" [1,H,S,T]
    ("vit_b16_b1", 1, 12, 197, 197, 64, None),
    ("vit_b16_b8", 8, 12, 197, 197, 64, None),
    ("deit_tiny_b1", 1, 3, 197, 197, 64, None),
    ("deit_tiny_b8", 8, 3, 197, 197, 64, None),
    ("mobilevit_64tok_d64", 4, 4, 64, 64, 64, None),
    ("enc_384tok_d64", 1, 8, 384, 384, 64, None),
    ("enc_512tok_d64", 1, 8, 512, 512, 64, None),
    ("enc_640tok_d64", 1, 8, 640, 640, 64, None),
    ("detr_850tok_d32", 1, 8, 850, 850, 32, None),
    ("detr_850tok_d32_mask", 1, 8, 850, 850, 32, "mask"),
    ("swin_t_s1_b1", 64, 3, 49, 49, 32, "rel"),
    ("swin_t_s1_b8", 512, 3, 49, 49, 32, "rel"),
    ("bert_base_128_b1", 1, 12, 128, 128, 64, "mask"),
    ("bert_base_128_b8", 8, 12, 128, 128, 64, "mask"),
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
    import attention_layout_cases as alc
    import cases
    import eltwise_cases
    from pool_cases import _q
    pkg = cases.pkg
    if a.lib:
        pkg.LIB_DIR = os.path.abspath(a.lib)
    hip = pkg.load_hip()
    if hip.shl_mi355x_device_count() < 1:
        raise SystemExit("attention_layout_bench: no MI355X visible: " + hip.shl_mi355x_last_error().decode())
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
            raise SystemExit("attention_layout_bench: graph capture failed: " + hip.shl_mi355x_last_error().decode())
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
        replays = max(20, int(np.ceil(20 * a.window_ms / max(window(ga, 20), window(gb, 20)))))
        wa, wb = [], []
        for _ in range(a.windows):
            wa.append(window(ga, replays))
            wb.append(window(gb, replays))
        hip.shl_mi355x_graph_destroy(ga)
        hip.shl_mi355x_graph_destroy(gb)
        per = 1e-3 / (replays * reps)
        return [(float(np.median(w)) * per, (max(w) - min(w)) * per) for w in (wa, wb)]

    head = ["shape", "images x heads x S x T x d", "bias", "dtype", "A: launches", "A us", "spread", "B (1) us", "spread", "B / A", "admit",
            "A': launches", "B / A'"]
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
            c.update(B=images, H=heads, pattern="reshape", gap=0, moved=alc.MOVED_ALL, offset=0, bias_geom=None)
            rng = ac._rng("attention layout bench " + c["name"])
            if kind:
                shape = (images, 1, 1, t) if kind == "mask" else (1, heads, s, t)
                c["bias_geom"] = "b_t" if kind == "mask" else "h_s_t"
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
            elems = dict(q=batches * s * d, k=batches * t * d, v=batches * t * d, out=batches * s * d)
            bufs = []
            for _ in range(SETS):
                b = {}
                for key in ("q", "k", "v"):
                    b["src_" + key] = dev.alloc(c[key].nbytes)
                    dev.upload(b["src_" + key], alc.source_of(c, key))
                    b["r_" + key], b[key] = dev.alloc(c[key].nbytes), dev.alloc(c[key].nbytes)
                b["c"] = dev.alloc(16)
                dev.upload(b["c"], c["c"])
                if kind:
                    b["bias"] = dev.alloc(c["bias"].nbytes)
                    dev.upload(b["bias"], c["bias"])
                for key in ("s", "x", "sum", "p"):
                    b[key] = dev.alloc(batches * s * t * es)
                for key in ("core", "t_out", "a_out", "b_out"):
                    b[key] = dev.alloc(elems["out"] * es)
                bufs.append(b)
            desc = ac.desc(c)
            qk, mul, pv = ac.unfused_descs(c)
            bd = add = None
            if kind:
                add = eltwise_cases.mul_desc(dict(dtype=dtype, in_q=c["sc_q"], in1_q=c["b_q"], out_q=c["sb_q"]), (images, heads, s, t), shape)
                bd = alc.bias_desc(c)
            ld = alc.layout_desc(hip, c)
            moves = {key: alc._mdesc(c, c[key + "_q"]) for key in ("q", "k", "v", "out")}
            rows = dict(q=s, k=t, v=t)
            split = {key: alc._tdesc(c, (images, rows[key], heads, d), (0, 2, 1, 3), c[key + "_q"]) for key in ("q", "k", "v")}
            merge = alc._tdesc(c, (images, heads, s, d), (0, 2, 1, 3), c["out_q"])
            b0 = bufs[0]
            if kind:
                by_default = hip.shl_mi355x_attention_bias_by_default(b0["q"], b0["k"], b0["v"], b0["bias"], b0["core"], C.byref(desc), C.byref(bd))
            else:
                by_default = hip.shl_mi355x_attention_by_default(b0["q"], b0["k"], b0["v"], b0["core"], C.byref(desc))

            def block(kk, fused_core):
                b = bufs[kk % SETS]
                for key in ("q", "k", "v"):
                    pkg.check(hip.shl_mi355x_move(b["src_" + key], b["r_" + key], elems[key], C.byref(moves[key]), stream), hip, "move")
                    pkg.check(hip.shl_mi355x_transpose(b["r_" + key], b[key], C.byref(split[key]), stream), hip, "transpose")
                if fused_core and kind:
                    pkg.check(hip.shl_mi355x_attention_bias(b["q"], b["k"], b["v"], b["bias"], b["core"], C.byref(desc), C.byref(bd), stream),
                              hip, "attention_bias")
                elif fused_core:
                    pkg.check(hip.shl_mi355x_attention(b["q"], b["k"], b["v"], b["core"], C.byref(desc), stream), hip, "attention")
                else:
                    pkg.check(hip.shl_mi355x_matmul(b["q"], b["k"], b["s"], C.byref(qk), stream), hip, "matmul (q k^T)")
                    pkg.check(hip.shl_mi355x_mul(b["s"], b["c"], b["x"], C.byref(mul), stream), hip, "mul")
                    x, x_q = b["x"], c["sc_q"]
                    if kind:
                        pkg.check(hip.shl_mi355x_add_bcast(b["x"], b["bias"], b["sum"], C.byref(add), stream), hip, "add_bcast")
                        x, x_q = b["sum"], c["sb_q"]
                    pkg.check(hip.shl_mi355x_softmax(x, b["p"], code, batches * s, t, 1, x_q[0], x_q[1], c["p_q"][0], c["p_q"][1], stream), hip,
                              "softmax")
                    pkg.check(hip.shl_mi355x_matmul(b["p"], b["v"], b["core"], C.byref(pv), stream), hip, "matmul (p v)")
                pkg.check(hip.shl_mi355x_transpose(b["core"], b["t_out"], C.byref(merge), stream), hip, "transpose (back)")
                pkg.check(hip.shl_mi355x_move(b["t_out"], b["a_out"], elems["out"], C.byref(moves["out"]), stream), hip, "move (back)")

            def layout(kk):
                b = bufs[kk % SETS]
                pkg.check(hip.shl_mi355x_attention_layout(b["src_q"], b["src_k"], b["src_v"], b["bias"] if kind else None, b["b_out"],
                                                          C.byref(desc), C.byref(bd) if kind else None, C.byref(ld), stream), hip,
                          "attention_layout")

            def fetch(p):
                pkg.check(hip.shl_mi355x_stream_sync(stream), hip, "sync")
                return dev.download(p, (elems["out"],), c["q"].dtype).view(np.uint8 if es == 1 else np.uint16)
            core_launches = lambda fused_core: 1 if fused_core else (5 if kind else 4)
            cells = [name, "%d x %d x %d x %d x %d" % (images, heads, s, t, d), {None: "-", "mask": "[B,1,1,T]", "rel": "[1,H,S,T]"}[kind], dtype]
            if hip.shl_mi355x_attention_layout_kernel_name(b0["src_q"], b0["src_k"], b0["src_v"], b0["bias"] if kind else None, b0["b_out"],
                                                           C.byref(desc), C.byref(bd) if kind else None, C.byref(ld)) == b"":
                cells += ["-", "-", "-", "no kernel: " + hip.shl_mi355x_last_error().decode(), "-", "-", "-", "-", "-"]
            else:
                for fused_core in (False, True):
                    block(0, fused_core)
                    want = fetch(b0["a_out"])
                    layout(0)
                    if not np.array_equal(fetch(b0["b_out"]), want):
                        raise SystemExit("attention_layout_bench: %s %s: the layout launch differs from the launches it replaces" % (name, dtype))
                dflt = bool(by_default)
                (t_a, r_a), (t_b, r_b) = alternate(lambda kk: block(kk, dflt), layout, a.reps)
                (t_o, _), (t_b2, _) = alternate(lambda kk: block(kk, not dflt), layout, a.reps)
                admit = t_b < t_a and (t_a - t_b) > max(r_a, r_b)
                cells += ["8 + %d" % core_launches(dflt), "%.2f" % (t_a * 1e6), "%.2f us" % (r_a * 1e6), "%.2f" % (t_b * 1e6),
                          "%.2f us" % (r_b * 1e6), "%.2f" % (t_b / t_a), "yes" if admit else "no", "8 + %d" % core_launches(not dflt),
                          "%.2f" % (t_b2 / t_o)]
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
