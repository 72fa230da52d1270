#!/usr/bin/env python3
"""bench.py — images/s of the WeDetect hot path on MI355X (BASELINE.json configs[1]).

    python bench.py --gpus N --steps K --warmup W
    N > 1: one rank per GPU over RCCL.  Started under torch.distributed.run (RANK / WORLD_SIZE in the environment) it
    is one of the N ranks; started plainly (`python bench.py --gpus 8`) it launches the N ranks itself — the same
    torch.distributed.run command line the reference's dist_test.sh:11-22 / extract_embedding.py:1665-1669 use — and
    relays their single JSON line.  It never reports n_gpus < N.

One step = one pass of the hot path over one batch of synthetic images already resident in
HBM as uint8 NHWC: ConvNeXt-Base tower + CSPRepBiFPAN neck + YOLO-World head (region
embeddings, DFL boxes) -> L2-normalised 80-class text bank similarity GEMM (+ per-level
scale/bias + sigmoid) -> score filter (> 0.001) / top-30000 / sort -> class-aware NMS (0.7)
-> <= 300 detections + their 768-d embeddings per image, all on device.  At N > 1 every
rank runs that on its own batch (images shard with no data-path collective) and the
kept-region embeddings are exchanged with one all_gather_into_tensor per step (the
retrieval gather, extract_embedding.py:1753-1756).  Weights/images/text are seeded
synthetic (no checkpoints or datasets offline).  The steps are issued back to back: the top-k / NMS
kernels of step i (and, at N > 1, its region gather) go to the tower's second stream and run beside
the backbone of step i + 1 (ImageTower.detect(overlap_post=True); --no-overlap-post keeps every
kernel of a step on one stream).  Every step's post-process completes inside the timed bracket —
the closing torch.cuda.synchronize() drains both streams.

Prints ONE JSON line (rank 0) with the driver's contract (metric, value, unit, n_gpus, steps, warmup, ms_per_step,
higher_is_better, dtype, config; at N > 1 also per_rank below).  A plain run does only that: set-up, warm-up, the
timed steps, the line.  --dump-outputs DIR also writes what the last timed step returned (write_outputs).
--full adds the side measurements, all after the timed steps (retrieval mode: its cpu_baseline):
  roofline      — the dominant kernel (the GEMM that runs the ConvNeXt MLPs: fp16x3 direct-to-LDS, or fp32 MFMA),
                  algorithmic flops / HIP-event time of its launches inside the timed region (events stamped by the
                  kernels' own dispatches, on the last two timed steps: see GemmTimer)
  sim_gemm      — the judged region x text similarity GEMM, same accounting
  fp32_mode     — (default fp16x3 arithmetic only) the same workload re-timed in this run with native fp32 MFMA,
                  and the max |difference| of the fp16x3 step's embeddings / scores from it
  cpu_baseline  — the CPU oracle (port of the reference's PyTorch-CPU path) on a bounded sample
  host_fed      — (N = 1) the same step fed from PINNED HOST memory: the uint8 batch is uploaded every step and the
                  <= 300-row results (boxes, scores, labels, counts) are copied back, both on a copy stream that
                  overlaps the next / previous step's compute; never the headline `value`
  other_configs — (N = 1, the default configuration) short runs of configs[2] / [3] / [4]
and, with or without --full:
  per_rank      — (N > 1) every rank's own ms/step and how long its stream stalled on the region gather
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, dense
F16_MFMA_PEAK_TFLOPS = 2516.6    # MI355X_MICROARCH.md: fp16/bf16 dense (v_mfma_f32_32x32x16_f16)
PEAK_CLOCK_MHZ = 2400.0          # the clock those peaks are quoted at
SPLIT_PASSES = 3                 # fp16x3: hi*hi + hi*lo + lo*hi per fp32-accurate product
SIM_SPLIT_TAG = "fp16x3 256x256x32/8w/p8/similarity"     # wd_similarity_split (round 6: banks of >= 256 rows)
HBM_PEAK_TBS = 8.0               # MI355X_MICROARCH.md
# bench tag -> kernel symbol in the rocprofv3 traces / profiles/r01_traffic.json
KERNEL_SYMBOL = {
    "128x128x16/8w/plain": "conv_gemm_kernel<2, 4, 4, 2, false, 16, 256>",
    "128x128x16/8w/conv": "conv_gemm_kernel<2, 4, 4, 2, true, 16, 256>",
    "64x128x16/4w/plain": "conv_gemm_kernel<2, 4, 2, 2, false, 16, 256>",
    "64x128x16/4w/conv": "conv_gemm_kernel<2, 4, 2, 2, true, 16, 256>",
    "64x80x32/4w/plain": "conv_gemm_kernel<1, 5, 4, 1, false, 32, 258>",
    "fp16x3 128x128x16/4w/plain": "split_gemm_kernel<2, 2, 2, 2, 16, false, 770>",
    "fp16x3 128x128x16/4w/conv": "split_gemm_kernel<2, 2, 2, 2, 16, true, 770>",
    "fp16x3 128x128x32/4w/plain": "split_gemm_kernel<2, 2, 2, 2, 32, false, 770>",
    "fp16x3 128x128x32/4w/conv": "split_gemm_kernel<2, 2, 2, 2, 32, true, 770>",
    "fp16x3 128x128x32/4w/pf2/plain": "split_gemm_kernel<2, 2, 2, 2, 32, false, 896>",
    # one bench tag, two instantiations: pwconv1 (output written as fp16 hi/lo groups) and pwconv2
    "fp16x3 128x128x16/4w/glds/plain": ["split_gemm_glds_kernel<16, 2048>", "split_gemm_glds_kernel<16, 0>"],
    "fp16x3 256x128x16/8w/pingpong/plain": ["split_gemm_pingpong_kernel<2048, 3, 2>", "split_gemm_pingpong_kernel<0, 3, 2>"],
    "fp16x3 128x256x16/4w/p4/plain": ["split_gemm_p4_kernel<2048>", "split_gemm_p4_kernel<0>"],
    "fp16x3 256x256x32/8w/p8s/plain": ["split_gemm_p8_kernel<2048, 0, true>", "split_gemm_p8_kernel<0, 0, true>"],
    # tile form and gang-scheduled persistent form (the default where it applies since round 4) of both epilogue variants
    "fp16x3 256x256x32/8w/p8/plain": ["split_gemm_p8_kernel<2048, 0, false>", "split_gemm_p8_kernel<0, 0, false>",
                                      "split_gemm_p8_kernel<2048, 0, true>", "split_gemm_p8_kernel<0, 0, true>"],
    "fp16x3 256x128x16/8w/dma/conv": ["split_conv_pp_kernel<3, 2, true, 0>", "split_conv_pp_kernel<4, 2, true, 0>"],
    # round 6: the 3 x 3 / stride 1 layers — twelve-wave producer / consumer kernel; the narrow layers with more tiles than CUs on the
    # eight-wave ring-of-two form
    "fp16x3 256x128x16/12w/dma3/conv": ["split_conv3w_kernel<2, true>", "split_conv3w_kernel<2, false>"],
    "fp16x3 256x64x16/12w/dma3/conv": ["split_conv3w_kernel<1, true>", "split_conv3w_kernel<1, false>"],
    "fp16x3 256x64x16/8w/dma3/ring2/conv": ["split_conv3_kernel<1, true, 2, false>", "split_conv3_kernel<1, false, 2, false>"],
}


def power_ceiling():
    """What the dominant kernel's K loop sustains on this chip with NO epilogue (VERDICT r5 #2a; scripts/p8_ceiling.py on an ablation
    build, random data, 0.4 s of back-to-back launches per arm, shader clock sampled): the committed measurement, not a live one —
    the ablation kernels are not part of the release library."""
    path = os.path.join(ROOT, "profiles", "r06_p8_power_ceiling.jsonl")
    try:
        rows = [json.loads(l) for l in open(path) if l.strip()]
        loop = [r for r in rows if r.get("kernel", "").startswith("k-loop only")]
        by = {r["arm"].split()[0]: r for r in loop}
        return {"frac": round(sum(r["frac_of_fp16x3_roof"] for r in (by["pw1"], by["pw2"])) / 2, 4),
                "pwconv1_k_loop": {k: by["pw1"][k] for k in ("avg_us", "tflops", "frac_of_fp16x3_roof", "effective_mhz", "frac_at_effective_clock")},
                "pwconv2_k_loop": {k: by["pw2"][k] for k in ("avg_us", "tflops", "frac_of_fp16x3_roof", "effective_mhz", "frac_at_effective_clock")},
                "meaning": "fraction of the fp16x3 roof (2516.6 / 3 TF at 2.4 GHz) the 256 x 256 K loop reaches with its epilogue removed, "
                           "stage-3 shapes of this workload: the chip sustains 1.6 - 1.75 GHz in it (power); `frac` above is the same "
                           "kernel WITH its epilogues inside the step",
                "source": "profiles/r06_p8_power_ceiling.jsonl (scripts/p8_ceiling.py, -DWD_DEBUG_ABLATIONS build)"}
    except Exception as ex:                      # the file is evidence, not a dependency of the measurement
        return {"frac": None, "source": f"profiles/r06_p8_power_ceiling.jsonl unreadable: {ex}"}


def measured_traffic(tag):
    """HBM bytes per launch from the committed PMC passes (profiles/r06_traffic.json, else r05 ... r02, for the fp16x3
    build; profiles/r01_traffic.json for the fp32 build: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of this same
    command, FETCH_SIZE doubled per MI355X_MICROARCH.md) — PMC passes cannot run inside the timed process, so the figure
    comes from a file, and its PROVENANCE is returned with it: the file, the commit and kernel-source hash it was taken
    at, and whether that hash equals the sources of the library that is running now.  (None, None) when no PMC record
    matches the kernel that ran."""
    from wedetect_amd.build import source_hash
    syms = KERNEL_SYMBOL.get(tag)
    if syms is None:
        return None, None
    syms = [syms] if isinstance(syms, str) else syms
    for name in (("r06_traffic.json", "r05_traffic.json", "r04_traffic.json", "r03_traffic.json", "r02_traffic.json", "r01_fp16x3_traffic.json")
                 if tag.startswith("fp16x3") else ("r01_traffic.json",)):
        try:
            doc = json.load(open(os.path.join(ROOT, "profiles", name)))
            rec = doc["kernels"]
            present = [s_ for s_ in syms if s_ in rec]            # the instantiations that ran in the profiled step (per FILE:
            if not present:                                       # an older file is still tried with the full symbol list)
                continue
            n = sum(rec[s_]["launches"] for s_ in present)
            val = round(sum(rec[s_]["hbm_bytes_per_launch"] * rec[s_]["launches"] for s_ in present) / n)
            now = source_hash()
            return val, {"file": f"profiles/{name}", "commit": doc.get("commit"), "kernel_source_sha256": doc.get("kernel_source_sha256"),
                         "running_kernel_source_sha256": now, "taken_on_these_sources": doc.get("kernel_source_sha256") == now}
        except Exception:
            continue
    return None, None
HBM_PEAK_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)      # >= 50 timed iterations after >= 10 warm-ups
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--arch", default="base")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--classes", type=int, default=None, help="text bank size (default 80; 1 000 000 in --mode retrieval)")
    ap.add_argument("--regions", type=int, default=300, help="--mode retrieval: kept regions per image")
    ap.add_argument("--mode", choices=["detect", "uni", "retrieval"], default="detect",
                    help="detect: normalised text bank, thr 0.001, rescale-before-NMS (configs[1]); "
                         "uni: WeDetect-Uni prompts as stored, thr 0.0, NMS in network pixels (configs[3]); "
                         "retrieval: the object-retrieval scoring step of configs[4] — 300 kept regions per image against a "
                         "1M-class bank, class-sharded over the ranks (retrieval_metric.py:367-377)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short legs of configs[2] / [3] / [4] that the --full line carries in `other_configs` (N = 1 only)")
    ap.add_argument("--precision", choices=["fp32", "fp16x3"], default=None,
                    help="arithmetic of the dense convs/linears (default: wedetect_amd.engine.DEFAULT_PRECISION); "
                         "fp16x3 = fp32 operands split into fp16 hi+lo, three MFMA passes, fp32 accumulate")
    ap.add_argument("--split-k", action="store_true",
                    help="latency mode: let under-filled fp16x3 launches split K (helps small batches; see engine.ImageTower)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-fp32-reference", action="store_true",
                    help="skip the short native-fp32 run that is reported beside an fp16x3 result (N = 1 only)")
    ap.add_argument("--no-host-fed", action="store_true", help="skip the host-fed (PCIe-inclusive) leg (N = 1 only)")
    ap.add_argument("--no-overlap-post", action="store_true",
                    help="issue top-k / NMS on the main stream, in front of the next step's backbone (default: on the tower's "
                         "second stream, beside it)")
    ap.add_argument("--no-calibrate", action="store_true",
                    help="skip the untimed range-calibration pass (an fp32 run of the tower): keeps it out of a rocprofv3 trace")
    ap.add_argument("--cpu-runs", type=int, default=5, help="timed CPU-oracle passes per leg (median reported; 3 warm-ups)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: per-kernel figures (roofline, gemm_kernels, sim_gemm, from the serial "
                         "leg), fp32_mode, host_fed, other_configs, cpu_baseline.  Off: set-up, warm-up, the timed steps, the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (float32 / float64, "
                         "<= 64 MB in all; the inputs are seeded, so two builds can be compared output for output)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if a.classes is None:
        a.classes = 1_000_000 if a.mode == "retrieval" else 80
    return a


class GemmTimer:
    """Per-launch durations of the wd_conv_gemm launches inside the timed region, without disturbing it: every
    launch carries a pre-created HIP event pair that the kernel's own dispatch stamps with its begin / end
    (wd_time_next_gemm -> hipExtLaunchKernelGGL on the launch stream).  An hipEventRecord pair around each launch
    would add ~5 us of idle per launch — 1.2 ms to this 48 ms step (scripts/step_timer_overhead.py).
    mode: "off" | "count" (warm-up: how many launches a step makes) | "time"."""

    def __init__(self, lib):
        self.lib = lib
        self.rec = {}          # tag -> list of (start, end, flops, bytes)
        self.mode = "off"
        self.count = 0
        self.pool = []
        self._orig = lib.conv_gemm
        self._orig_mlp = lib.mlp_fused
        self._orig_mlpw = lib.mlp_fused_wide
        self._orig_sim = lib.similarity_split
        self._orig_mlpw_ln = lib.mlp_fused_wide_ln

    @staticmethod
    def _pair():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()             # creates the underlying hipEvent_t (torch does it lazily)
        e.record()
        return s, e

    def prepare(self, n_launches: int):
        """Event pairs for the timed region, created (and drained from the stream) before it starts."""
        self.pool = [self._pair() for _ in range(n_launches)]
        torch.cuda.synchronize()

    def install(self):
        orig, rec, lib = self._orig, self.rec, self.lib

        def wrapped(a, w, bias, c, **kw):
            if self.mode != "time":
                self.count += self.mode == "count"
                return orig(a, w, bias, c, **kw)
            kh, kw_ = kw.get("kh", 1), kw.get("kw", 1)
            hin, win, stride, pad = kw["hin"], kw["win"], kw.get("stride", 1), kw.get("pad", 0)
            hout = (hin + 2 * pad - kh) // stride + 1
            wout = (win + 2 * pad - kw_) // stride + 1
            m, n, k = kw["batch"] * hout * wout, kw["n"], kh * kw_ * kw["cin"]
            plain = kh == 1 and kw_ == 1 and stride == 1 and pad == 0
            ws_t = kw.get("workspace")
            park = ws_t is not None and bool(kw.get("split_flags", 0)) and ws_t.numel() * 4 == lib.p8_workspace_bytes()
            flags = kw.get("split_flags", 0)
            special = (kw.get("out_mode", 0) != 0 or kw.get("c_batch_stride", 0) > 0 or kw.get("seg") is not None or kw.get("sigmoid")
                       or kw.get("out_scale", 1.0) != 1.0 or kw.get("out_bias", 0.0) != 0.0)
            covered = plain and not special and kw.get("c2") is None and not ((flags & lib.SPLIT_C) and kw.get("res") is not None)
            dma = kw.get("w_split") is not None and bool(flags & lib.SPLIT_A) and not covered
            tag = lib.gemm_config(m, n, k, split=kw.get("w_split") is not None, conv=not plain,
                                  presplit=bool(flags & lib.SPLIT_A), park=park, dma=dma,
                                  conv3=dma and kh == 3 and kw_ == 3 and stride == 1 and pad == 1 and kw["cin"] % 16 == 0
                                  and os.environ.get("WEDETECT_CONV3", "1") != "0") + ("/plain" if plain else "/conv")
            if os.environ.get("WEDETECT_BENCH_BY_SHAPE") == "1":       # diagnostic: one line per layer shape
                tag += f" m{m} n{n} k{kh}x{kw_}x{kw['cin']} s{stride}" + (" ks2" if kw.get("k_splits") else "")
            s, e = self.pool.pop() if self.pool else self._pair()
            lib.time_next_gemm(s, e)
            orig(a, w, bias, c, **kw)
            # algorithmic HBM bytes: A (or the NHWC input once), W, C, residual — fp32
            a_elems = kw["batch"] * hin * win * kw["cin"]
            nbytes = 4.0 * (a_elems + n * k + m * n * (2 if kw.get("res") is not None else 1))
            rec.setdefault(tag, []).append((s, e, 2.0 * m * n * k, nbytes))
        lib.conv_gemm = wrapped
        orig_mlp = self._orig_mlp

        def wrapped_mlp(a_split, rows, c, hidden, *args, **kw):     # the one-kernel block MLP: two GEMMs' worth of flops
            if self.mode != "time":
                self.count += self.mode == "count"
                return orig_mlp(a_split, rows, c, hidden, *args, **kw)
            s, e = self.pool.pop() if self.pool else self._pair()
            lib.time_next_gemm(s, e)
            orig_mlp(a_split, rows, c, hidden, *args, **kw)
            nbytes = 4.0 * (3 * rows * c + 2 * c * hidden)           # LN rows in, x in and out, both weight matrices
            rec.setdefault("fp16x3 fused block MLP 128x(128->512->128)/4w/dma", []).append((s, e, 4.0 * rows * c * hidden, nbytes))
        lib.mlp_fused = wrapped_mlp
        orig_mlpw = self._orig_mlpw

        def wrapped_mlpw(a_split, rows, c, hidden, *args, **kw):    # round 4: the wide stages' block MLP as one kernel
            if self.mode != "time":
                self.count += self.mode == "count"
                return orig_mlpw(a_split, rows, c, hidden, *args, **kw)
            s, e = self.pool.pop() if self.pool else self._pair()
            lib.time_next_gemm(s, e)
            orig_mlpw(a_split, rows, c, hidden, *args, **kw)
            nbytes = 4.0 * (3 * rows * c + 2 * c * hidden)
            rec.setdefault(f"fp16x3 fused block MLP 128x({c}->{hidden}->{c})/4w/frag", []).append((s, e, 4.0 * rows * c * hidden, nbytes))
        lib.mlp_fused_wide = wrapped_mlpw
        orig_mlpw_ln = self._orig_mlpw_ln

        def wrapped_mlpw_ln(d_split, rows, c, hidden, *args, **kw):   # round 6: the same kernel with the LayerNorm folded in
            if self.mode != "time":
                self.count += self.mode == "count"
                return orig_mlpw_ln(d_split, rows, c, hidden, *args, **kw)
            s, e = self.pool.pop() if self.pool else self._pair()
            lib.time_next_gemm(s, e)
            orig_mlpw_ln(d_split, rows, c, hidden, *args, **kw)
            nbytes = 4.0 * (3 * rows * c + 2 * c * hidden)
            rec.setdefault(f"fp16x3 fused block MLP 128x({c}->{hidden}->{c})/4w/frag", []).append((s, e, 4.0 * rows * c * hidden, nbytes))
        lib.mlp_fused_wide_ln = wrapped_mlpw_ln
        orig_sim = self._orig_sim

        def wrapped_sim(e_split, rows, t_split, unscale, out, n_cls, dim, ldo, **kw):   # round 6: the similarity GEMM on the fp16x3 kernel
            if self.mode != "time":
                self.count += self.mode == "count"
                return orig_sim(e_split, rows, t_split, unscale, out, n_cls, dim, ldo, **kw)
            s, e = self.pool.pop() if self.pool else self._pair()
            lib.time_next_gemm(s, e)
            orig_sim(e_split, rows, t_split, unscale, out, n_cls, dim, ldo, **kw)
            nbytes = 4.0 * (rows * dim + n_cls * dim + rows * n_cls)
            rec.setdefault(SIM_SPLIT_TAG, []).append((s, e, 2.0 * rows * n_cls * dim, nbytes))
        lib.similarity_split = wrapped_sim

    def summary(self, busy: bool = False):
        out = {}
        merged = {}
        for tag, lst in self.rec.items():
            # the tile form and the persistent (gang-scheduled) form of the 256 x 256 kernel are one family: same tiles, same
            # MFMA chain, chosen per layer (K >= 512 and enough tiles -> persistent)
            merged.setdefault(tag.replace("/p8s/", "/p8/"), []).extend(lst)
        for tag, lst in merged.items():
            ms = sum(r[0].elapsed_time(r[1]) for r in lst)
            fl = sum(r[2] for r in lst)
            out[tag] = dict(launches=len(lst), ms_total=ms, flops_total=fl, bytes_total=sum(r[3] for r in lst),
                            avg_us=1e3 * ms / len(lst), tflops=fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0)
            if busy:
                # launches of one family on different streams overlap in time (image chains): the time during which AT LEAST ONE of
                # them was running = the union of their [begin, end] intervals on the device clock
                t0 = lst[0][0]
                out[tag]["busy_ms"] = union_length([(t0.elapsed_time(r[0]), t0.elapsed_time(r[1])) for r in lst])
        return out


def union_length(intervals) -> float:
    """Total length of the union of [begin, end] intervals (any order, may overlap or nest)."""
    iv = sorted(intervals)
    if not iv:
        return 0.0
    tot, (lo, hi) = 0.0, iv[0]
    for a_, b_ in iv[1:]:
        if a_ > hi:
            tot, lo, hi = tot + hi - lo, a_, b_
        else:
            hi = max(hi, b_)
    return tot + hi - lo


def timed_region_record(summ, dom_tag, peak, n_inst, tower):
    """The dominant kernel family as stamped INSIDE the timed region, where its launches run beside launches of other streams
    (the other image chain's, the previous step's neck / head): raw per-launch average (what a rocprofv3 trace of the default
    command shows) and the family's flops over the time at least one of its launches was running."""
    d = summ.get(dom_tag) or max(summ.values(), key=lambda v: v["flops_total"])
    fl, busy, n, ms = d["flops_total"], d.get("busy_ms", d["ms_total"]), d["launches"], d["ms_total"]
    pipe = bool(tower._pipe_neck_on())
    return {"backbones_in_flight": tower._bb_depth() if pipe else 1, "image_chains": 1 if pipe and tower._bb_depth() == 2 and tower.bb_chains == "auto" else tower._n_chains(),
            "neck_head_on_nh_stream": pipe,
            "launches_per_step": n // n_inst, "avg_launch_us_raw": round(1e3 * ms / max(1, n), 2),
            "algorithmic_gflop_per_launch": round(fl / max(1, n) / 1e9, 3),
            "busy_ms_per_step": round(busy / n_inst, 3),
            "achieved_over_busy_time": round(fl / (busy * 1e-3) / 1e12, 2) if busy > 0 else None,
            "frac_over_busy_time": round(fl / (busy * 1e-3) / 1e12 / peak, 4) if busy > 0 else None,
            "note": "busy time = union of the family's [begin, end] stamps on the device clock; other kernels run inside it"}


class ClockSampler:
    """Shader clock of the benchmarked device during the timed region, from the driver's own sysfs node
    (/sys/class/drm/card*/device/pp_dpm_sclk: the starred line is the current GFX clock), sampled every 10 ms by a host
    thread.  The dominant kernels run power-limited (1.8 - 2.0 GHz against the 2.4 GHz the MFMA peaks are quoted at); this
    puts that figure into the bench line itself instead of deriving it from GRBM_GUI_ACTIVE in a separate profile."""

    def __init__(self, device_index: int):
        import glob
        self.path, self.samples, self._stop, self._th = None, [], False, None
        try:
            p = torch.cuda.get_device_properties(device_index)
            want = f"{int(getattr(p, 'pci_domain_id', 0)):04x}:{int(p.pci_bus_id):02x}:{int(p.pci_device_id):02x}."
            for node in sorted(glob.glob("/sys/class/drm/card*/device")):
                if os.path.basename(os.path.realpath(node)).startswith(want) and os.path.exists(node + "/pp_dpm_sclk"):
                    self.path = node + "/pp_dpm_sclk"
                    break
        except Exception:
            self.path = None

    def _read(self):
        try:
            for line in open(self.path).read().splitlines():
                if line.rstrip().endswith("*"):
                    return float(line.split(":")[1].strip().split("M")[0])
        except Exception:
            pass
        return None

    def start(self):
        import threading
        if self.path is None:
            return

        def loop():
            while not self._stop:
                v = self._read()
                if v is not None:
                    self.samples.append(v)
                time.sleep(0.01)
        self._th = threading.Thread(target=loop, daemon=True)
        self._th.start()

    def stop(self):
        self._stop = True
        if self._th is not None:
            self._th.join(timeout=1.0)
        busy = [v for v in self.samples if v > 600.0]            # drop the idle / sleep states around the region
        if not busy:
            return None
        return {"mean_mhz": round(sum(busy) / len(busy), 1), "min_mhz": min(busy), "max_mhz": max(busy), "samples": len(busy),
                "source": self.path}


def usable_cores() -> int:
    """Host cores this process may actually use: affinity mask capped by the cgroup CPU quota
    (the GPU box exposes 256 logical CPUs but a 16-CPU quota; oversubscribing it is ~50x slower)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def cpu_baseline(arch, size, classes, runs):
    """The oracle (CPU port of the reference's PyTorch path) on a bounded sample, SURVEY.md 8(d) protocol: all usable
    host cores, the same synthetic workload at B = 1 (3 warm-ups + ``runs`` timed passes) and B = 8 (1 warm-up + 3 timed
    passes), MEDIAN reported.  ``value`` is the better of the two legs in images/s."""
    from oracle import postprocess as opp
    from oracle import ref_cpu as orc
    from wedetect_amd import weights as W
    from wedetect_amd.arch import get_arch
    torch.set_num_threads(usable_cores())
    a = get_arch(arch)
    sd = orc.to_torch(W.make_state_dict(arch))
    text = torch.from_numpy(W.make_text_bank(classes))
    imgs = W.make_images(8, size, size)

    def one_pass(b, i0):
        t0 = time.perf_counter()
        _, p = orc.forward_features(sd, a, imgs[i0:i0 + b])
        flat = orc.head_flat(sd, p, text, normalize_text=True)
        for i in range(b):
            opp.mmdet_predict_image(flat["boxes"][i].numpy(), flat["scores"][i].numpy(), None, (1.0, 1.0), (size, size))
        return time.perf_counter() - t0
    legs = {}
    with torch.no_grad():
        for b, warm, timed in ((1, 3, runs), (8, 1, 3)):
            ts = [one_pass(b, i % (8 // b) * b) for i in range(warm + timed)][warm:]
            legs[f"b{b}"] = {"images_per_s": round(b / float(np.median(ts)), 4), "median_s_per_pass": round(float(np.median(ts)), 4),
                             "timed_passes": timed, "warmups": warm}
    best = max(legs.values(), key=lambda v: v["images_per_s"])
    return dict(value=best["images_per_s"], unit="images/s", cores=torch.get_num_threads(), kind="port", legs=legs,
                sample=f"the same {arch}@{size} K={classes} path (oracle/ref_cpu.py + oracle/postprocess.py: network, mmcv-form NMS; "
                       f"fp32, torch {torch.__version__}) at batch 1 ({runs} timed passes after 3 warm-ups) and batch 8 (3 after 1); "
                       f"median per leg, value = the faster leg")


def fp32_reference_run(args, tower, images, text, meta, uni, steps=10):
    """``steps`` timed steps of the identical workload on a second tower in fp32 mode (sharing the packed
    weights), issued like the headline's (a stream of batches: detect(overlap_post=True); round 6 — the in-line form of
    rounds 1-5 measured 354 images/s where the pipelined one gives 374), plus how far the fp16x3 step's outputs are from it."""
    from wedetect_amd.engine import ImageTower
    ref = ImageTower(args.arch, tower.P, tower.B, tower.H, tower.W, max_classes=tower.max_classes, precision="fp32")
    kw = dict(normalize_text=not uni, score_thr=0.0 if uni else 0.001, with_embed=True, overlap_post=True)
    emb16 = tower.embed.clone()
    sc16 = tower.scores.view(-1)[: tower.B * tower.ntot * text.shape[0]].clone()
    for _ in range(3):
        ref.detect(images, text, meta, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ref.detect(images, text, meta, **kw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    d_emb = float((ref.embed - emb16).abs().max())
    d_sc = float((ref.scores.view(-1)[: sc16.numel()] - sc16).abs().max())
    return {"value": round(tower.B / dt, 3), "unit": "images/s", "ms_per_step": round(1e3 * dt, 3), "steps": steps,
            "dtype": "f32 (v_mfma_f32_16x16x4_f32)", "max_abs_diff_of_fp16x3_step": {"embeddings": d_emb, "scores": d_sc}}


def host_fed_run(tower, images, text, meta, uni, steps):
    """The same step with the batch coming from (and the results going back to) pinned host memory every step.
    Two device input buffers; uploads and result downloads run on a copy stream and overlap compute, the steps themselves
    are the pipelined ones of the headline (detect(overlap_post=True): results staged out on the tower's post stream):
        copy stream :  H2D batch i+1 | D2H results i-1
        tower       :  step i (backbone | neck + head | post-process on their streams)
    Measured over ``steps`` steps after 2 warm-ups, wall clock around a full drain."""
    dev = images.device
    B = images.shape[0]
    h_img = images.cpu().pin_memory()
    d_in = [torch.empty_like(images), torch.empty_like(images)]
    res0 = tower.detect(images, text, meta, normalize_text=not uni, score_thr=0.0 if uni else 0.001, with_embed=True)
    keys = ("bboxes", "scores", "labels", "count")
    h_out = {k: torch.empty(res0[k].shape, dtype=res0[k].dtype).pin_memory() for k in keys}
    d_out = [{k: torch.empty_like(res0[k]) for k in keys} for _ in range(2)]     # results staged out of the tower's buffers
    cs = torch.cuda.Stream(device=dev)
    main = torch.cuda.current_stream()
    up = [torch.cuda.Event(), torch.cuda.Event()]
    free_in = [torch.cuda.Event(), torch.cuda.Event()]
    done = [torch.cuda.Event(), torch.cuda.Event()]
    drained = [torch.cuda.Event(), torch.cuda.Event()]
    kw = dict(normalize_text=not uni, score_thr=0.0 if uni else 0.001, with_embed=True)

    def run(n):
        with torch.cuda.stream(cs):
            d_in[0].copy_(h_img, non_blocking=True)
            up[0].record(cs)
        for i in range(n):
            cur, nxt = i & 1, (i + 1) & 1
            if i + 1 < n:
                with torch.cuda.stream(cs):
                    if i >= 1:
                        cs.wait_event(free_in[nxt])            # step i-1 has finished reading that input buffer
                    d_in[nxt].copy_(h_img, non_blocking=True)
                    up[nxt].record(cs)
            main.wait_event(up[cur])
            r = tower.detect(d_in[cur], text, meta, overlap_post=True, **kw)
            free_in[cur].record(main)                          # the backbone (or its staging copy) is ordered on the caller's stream
            with torch.cuda.stream(tower.post_stream):         # the results are produced there
                if i >= 2:
                    tower.post_stream.wait_event(drained[cur])     # the D2H of step i-2 has left this staging set
                for k in keys:
                    d_out[cur][k].copy_(r[k], non_blocking=True)
                done[cur].record(tower.post_stream)
            with torch.cuda.stream(cs):
                cs.wait_event(done[cur])
                for k in keys:
                    h_out[k].copy_(d_out[cur][k], non_blocking=True)
                drained[cur].record(cs)
        torch.cuda.synchronize()

    run(2)
    t0 = time.perf_counter()
    run(steps)
    dt = (time.perf_counter() - t0) / steps
    h2d = h_img.numel()
    d2h = sum(v.numel() * v.element_size() for v in h_out.values())
    return {"value": round(B / dt, 3), "unit": "images/s", "ms_per_step": round(1e3 * dt, 3), "steps": steps,
            "h2d_bytes_per_step": int(h2d), "d2h_bytes_per_step": int(d2h),
            "note": "uint8 batch uploaded from pinned host memory and boxes / scores / labels / counts copied back EVERY step, "
                    "on a copy stream overlapped with compute (double-buffered); PCIe-inclusive, never the headline value",
            "kept_rows_last_image": int(h_out["count"][-1])}


def sim_record(summ, L, rows, K):
    """The similarity GEMM of the step that was timed: the kernel the DEFAULT path ran (fp32 MFMA for small banks, the fp16x3
    256 x 256 kernel from 256 classes), its algorithmic TFLOP/s against that arithmetic's MFMA roof — and against the HBM roof
    (embeddings + bank + scores, each once) where that is the tighter one: `bound` says which."""
    flops, nbytes = 2.0 * rows * K * 768, 4.0 * (rows * 768 + K * 768 + rows * K)
    for tag, peak, dtype in ((SIM_SPLIT_TAG, F16_MFMA_PEAK_TFLOPS / SPLIT_PASSES, "fp16x3"),
                             (L.gemm_config(rows, K, 768) + "/plain", F32_MFMA_PEAK_TFLOPS, "fp32")):
        r = summ.get(tag)
        if r is None:
            continue
        t_mfma, t_hbm = flops / (peak * 1e12), nbytes / (HBM_PEAK_TBS * 1e12)
        rec = {"kernel": tag, "dtype": dtype, "m": rows, "n": K, "k": 768, "achieved": round(r["tflops"], 2), "peak": round(peak, 1),
               "unit": "TFLOP/s", "frac": round(r["tflops"] / peak, 4), "avg_launch_us": round(r["avg_us"], 2),
               "bound": "hbm" if t_hbm > t_mfma else "mfma", "hbm_floor_us": round(1e6 * t_hbm, 1), "mfma_floor_us": round(1e6 * t_mfma, 1),
               "frac_of_tighter_roof": round(max(t_mfma, t_hbm) / (r["avg_us"] * 1e-6), 4)}
        return rec
    return None


def fp32_sim_reference(tower, L, text, normalize, reps=5):
    """The fp32-MFMA similarity launch on the same embeddings (the figure the north star's 0.6 target is quoted on), timed beside
    a step that ran the fp16x3 kernel: HIP events around ``reps`` launches on the current stream."""
    saved = tower._embed_split_valid
    tower._embed_split_valid = False
    try:
        for _ in range(2):
            tower.similarity(text, normalize=normalize)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            tower.similarity(text, normalize=normalize)
        e.record()
        torch.cuda.synchronize()
    finally:
        tower._embed_split_valid = saved
    us = 1e3 * s.elapsed_time(e) / reps
    rows, K = tower.B * tower.ntot, text.shape[0]
    tf = 2.0 * rows * K * 768 / us / 1e6
    return {"kernel": L.gemm_config(rows, K, 768) + "/plain", "dtype": "fp32", "avg_launch_us": round(us, 2), "achieved": round(tf, 2),
            "peak": F32_MFMA_PEAK_TFLOPS, "frac": round(tf / F32_MFMA_PEAK_TFLOPS, 4)}


def detect_leg(timer, L, arch, B, K, uni, steps=20, warmup=3):
    """A short run of ANOTHER BASELINE configuration inside a --full invocation (configs[2] / [3] were
    builder-run files only): same protocol as the headline — calibration, ``warmup`` untimed steps, ``steps`` timed steps
    issued back to back with the post-process on the second stream, wall clock around a full drain — and the per-launch
    GEMM timing on the last step for the similarity GEMM's fraction."""
    from wedetect_amd import weights as W
    from wedetect_amd.engine import ImageTower
    from wedetect_amd.pack import pack
    S = 640
    tower = ImageTower(arch, pack(W.make_state_dict(arch), arch), B, S, S, max_classes=K)
    images = torch.from_numpy(W.make_images(B, S, S, seed=1234)).cuda()
    text = torch.from_numpy(W.make_text_bank(K)).cuda()
    meta = tower.identity_meta()
    if not uni:
        meta[:, 7] = 1.0
    kw = dict(normalize_text=not uni, score_thr=0.0 if uni else 0.001, with_embed=True, overlap_post=True)
    tower.calibrate(images)
    timer.rec.clear()
    timer.count, timer.mode = 0, "count"
    for _ in range(warmup):
        tower.detect(images, text, meta, **kw)
    torch.cuda.synchronize()
    timer.prepare(timer.count // max(1, warmup))
    timer.mode = "off"
    t0 = time.perf_counter()
    for i in range(steps):
        if i == steps - 1:
            timer.mode = "time"
        res = tower.detect(images, text, meta, **kw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    timer.mode = "off"
    if tower._n_chains() > 1 or tower._pipe_neck_on():
        # per-kernel figures from a serial step (see main(): in the pipelined steps launches of several streams share the chip)
        timer.rec.clear()
        tower.bb_chains, tower.pipe_neck, tower.force_tile_forms = "1", "0", True
        tower.detect(images, text, meta, **kw)
        torch.cuda.synchronize()
        timer.prepare(timer.count // max(1, warmup))
        timer.mode = "time"
        tower.detect(images, text, meta, **kw)
        torch.cuda.synchronize()
        timer.mode = "off"
    summ = timer.summary()
    timer.rec.clear()
    out = {"workload": f"WeDetect-{arch.capitalize()}{'-Uni' if uni else ''}, batch {B}x{S}x{S}, {K}-class similarity, mode "
                       f"{'uni' if uni else 'detect'}", "value": round(B / dt, 3), "unit": "images/s", "ms_per_step": round(1e3 * dt, 3),
           "steps": steps, "warmup": warmup, "kept_regions_last_step": int(res["count"].sum().item()),
           "fp16x3_range_guard_tripped": bool(tower.range_flags.any().item())}
    sim = sim_record(summ, L, B * tower.ntot, K)
    if sim is not None:
        out["sim_gemm"] = sim
        if sim["dtype"] == "fp16x3":                       # keep the fp32-MFMA figure beside it
            out["sim_gemm"]["fp32_kernel"] = fp32_sim_reference(tower, L, text, not uni)
    if summ:
        dom_tag = max(summ, key=lambda k_: summ[k_]["flops_total"])
        if dom_tag.startswith("fp16x3"):
            out["dominant_gemm"] = {"tag": dom_tag, "avg_launch_us": round(summ[dom_tag]["avg_us"], 2),
                                    "frac": round(summ[dom_tag]["tflops"] / (F16_MFMA_PEAK_TFLOPS / SPLIT_PASSES), 4)}
    del tower
    torch.cuda.empty_cache()
    return out


BANK_SLICE = 125_000


def make_bank_rows(lo: int, hi: int, dim: int, device, seed: int = 4321) -> torch.Tensor:
    """Rows [lo, hi) of the synthetic unit-norm text bank (N(0, 1) rows, L2-normalised), generated on the
    device in fixed slices of 125 000 rows seeded by the slice index — the same bank whatever the class shard."""
    out = torch.empty(hi - lo, dim, dtype=torch.float32, device=device)
    for j in range(lo // BANK_SLICE, (hi + BANK_SLICE - 1) // BANK_SLICE):
        a, b = max(lo, j * BANK_SLICE), min(hi, (j + 1) * BANK_SLICE)
        g = torch.Generator(device=device).manual_seed(seed + j)
        blk = torch.nn.functional.normalize(torch.randn(BANK_SLICE, dim, device=device, generator=g), dim=-1)
        out[a - lo:b - lo] = blk[a - j * BANK_SLICE:b - j * BANK_SLICE]
        del blk
    return out


class RetrievalTimer:
    """HIP-event duration of the scoring kernel's own dispatch (wd_time_next_gemm), on selected steps."""

    def __init__(self, lib):
        self.lib, self.on, self.rec = lib, False, []
        self._orig = lib.retrieval_max_split

        def wrapped(*a, **kw):
            if not self.on:
                return self._orig(*a, **kw)
            s_, e_ = GemmTimer._pair()
            lib.time_next_gemm(s_, e_)
            self._orig(*a, **kw)
            self.rec.append((s_, e_))
        lib.retrieval_max_split = wrapped

    def avg_us(self):
        return 1e3 * sum(a.elapsed_time(b) for a, b in self.rec) / max(1, len(self.rec))

    def restore(self):
        self.lib.retrieval_max_split = self._orig


def retrieval_leg(L, n_img, regions, K, rank, world, steps, warmup, dist=None):
    """configs[4]: per step, the kept regions of ``n_img`` images per rank ([n_img, regions, 768] resident in HBM) are scored
    against a K-class bank — sigmoid(<e, t> exp(scale) + bias), max over an image's regions, logits never materialised
    (retrieval_metric.py:367-377).  N > 1: images AND the bank are sharded (parallel.class_sharded_retrieval: all-gather of
    the regions, every rank scores all images against its K / N classes, all-gather of the score blocks).  Returns the
    JSON pieces: seconds per step (max over ranks is the caller's), the kernel's average launch time and its work."""
    from wedetect_amd.parallel import BankScorer, class_sharded_retrieval, shard_range
    dev = torch.device("cuda", torch.cuda.current_device())
    D = 768
    g = torch.Generator(device=dev).manual_seed(777 + rank)
    e = torch.randn(n_img, regions, D, device=dev, generator=g) * 1.4
    sc = torch.randn(n_img, regions, device=dev, generator=g) * 0.1 - 0.35
    bi = torch.randn(n_img, regions, device=dev, generator=g) * 0.2 - 2.6
    cnt = torch.full((n_img,), regions, dtype=torch.int32, device=dev)
    mine = shard_range(K, world, rank)
    shard = make_bank_rows(mine.start, mine.stop, D, dev)
    scorer = BankScorer(shard)
    score_fn = lambda e_, c_, s_, b_, bank_: scorer(e_, c_, s_, b_, check=False)     # the range flag is read once, after the run
    rt = RetrievalTimer(L)

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
    for _ in range(warmup):
        out = class_sharded_retrieval(e, cnt, sc, bi, shard, K, score_fn=score_fn)
    sync()
    n_inst = min(steps, 2)
    clock = ClockSampler(dev.index)
    clock.start()
    t0 = time.perf_counter()
    for i in range(steps):
        rt.on = i >= steps - n_inst
        out = class_sharded_retrieval(e, cnt, sc, bi, shard, K, score_fn=score_fn)
    sync()
    dt = time.perf_counter() - t0
    clk = clock.stop()
    rt.on = False
    rt.restore()
    rows = world * n_img * regions
    flops = 2.0 * rows * len(mine) * D
    nbytes = 4.0 * (len(mine) * D + rows * D + world * n_img * len(mine))
    us = rt.avg_us()
    tf = flops / (us * 1e-6) / 1e12 if us > 0 else 0.0
    peak = round(F16_MFMA_PEAK_TFLOPS / SPLIT_PASSES, 1) if scorer.precision == "fp16x3" else F32_MFMA_PEAK_TFLOPS
    traffic, traffic_src = None, None
    if (world, n_img, regions, K, scorer.precision) == (1, 32, 300, 1_000_000, "fp16x3"):
        # fabric-side bytes per launch of THIS configuration from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE
        # over `bench.py --mode retrieval --steps 2 --warmup 1`): L2 misses, Infinity-Cache hits included — 5 passes over the
        # 3.07 GB bank (one per gang of eight row tiles) + the 29 MB of region rows re-fetched per four bank blocks; the kernel is
        # bound by its K loop, not by this traffic (1.25 TB/s)
        try:
            from wedetect_amd.build import source_hash
            doc = json.load(open(os.path.join(ROOT, "profiles", "r05_traffic_retrieval.json")))
            rec = doc["kernels"]["split_gemm_p8_kernel<4096, 0, false>"]
            traffic = round(rec["hbm_bytes_per_launch"])
            now = source_hash()
            traffic_src = {"file": "profiles/r05_traffic_retrieval.json", "commit": doc.get("commit"),
                           "kernel_source_sha256": doc.get("kernel_source_sha256"), "running_kernel_source_sha256": now,
                           "taken_on_these_sources": doc.get("kernel_source_sha256") == now,
                           "note": "FETCH_SIZE / WRITE_SIZE are fabric-side counters: Infinity-Cache hits are in them"}
        except Exception:
            traffic, traffic_src = None, None
    return dict(dt=dt, precision=scorer.precision, tripped=scorer.tripped(), checksum=float(out[:, :: max(1, K // 4096)].double().sum().item()),
                scores=out,
                roofline={"kernel": ("split_gemm_p8_kernel<retrieval: bank rows x region rows, fp16x3 256x256x32/8w, in-register max over "
                                     "regions + one sigmoid per (image, class)> (3 x v_mfma_f32_32x32x16_f16 per product)"
                                     if scorer.precision == "fp16x3" else "retrieval_max_kernel (fp32 MFMA 16x16x4)"),
                          "bound": "mfma", "achieved": round(tf, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(tf / peak, 4),
                          **({"effective_mhz": clk["mean_mhz"], "effective_mhz_min_max": [clk["min_mhz"], clk["max_mhz"]],
                              "peak_quoted_at_mhz": PEAK_CLOCK_MHZ,
                              "frac_at_effective_clock": round(tf / peak * PEAK_CLOCK_MHZ / clk["mean_mhz"], 4),
                              "clock_note": "shader clock from sysfs during the timed steps: this launch is power-limited "
                                            "(SQ counters: profiles/r05_rocprofv3_retrieval_sq.txt); frac stays against the spec peak"}
                             if clk else {"effective_mhz": None}),
                          "traffic": traffic, "traffic_provenance": traffic_src,
                          "timing": f"HIP events stamped by the kernel's own dispatch, last {n_inst} of the {steps} timed steps",
                          "avg_launch_us": round(us, 1), "launches_per_step": 1,
                          "algorithmic_gflop_per_launch": round(flops / 1e9, 2), "algorithmic_bytes_per_launch": int(nbytes),
                          "peak_note": (f"fp16 dense MFMA peak {F16_MFMA_PEAK_TFLOPS} / {SPLIT_PASSES} passes per product"
                                        if scorer.precision == "fp16x3" else "fp32 MFMA dense peak")})


def retrieval_cpu_baseline(regions, K, sample_images=2, sample_classes=100_000):
    """The oracle's retrieval lines (oracle/postprocess.py: retrieval_scores, the torch-fp32 op sequence of
    retrieval_metric.py:369-375) on a bounded sample: ``sample_images`` images x ``sample_classes`` classes, timed on the usable
    host cores; images/s at the full bank = the measured rate x sample_classes / K (the work is linear in the classes)."""
    from oracle import postprocess as opp
    torch.set_num_threads(usable_cores())
    g = np.random.default_rng(5)
    t = g.standard_normal((sample_classes, 768)).astype(np.float32)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    e = (g.standard_normal((sample_images, regions, 768)) * 1.4).astype(np.float32)
    sc = np.full(regions, -0.35, np.float32)
    bi = np.full(regions, -2.6, np.float32)
    opp.retrieval_scores(e[0], t, sc, bi)
    t0 = time.perf_counter()
    for i in range(sample_images):
        opp.retrieval_scores(e[i], t, sc, bi)
    per_img = (time.perf_counter() - t0) / sample_images
    return dict(value=round(sample_classes / K / per_img, 5), unit="images/s", cores=torch.get_num_threads(), kind="port",
                sample=f"oracle/postprocess.py retrieval_scores (torch fp32 einsum + sigmoid + max) on {sample_images} images x {regions} "
                       f"regions x {sample_classes} classes: {per_img:.3f} s per image; value = that rate scaled to {K} classes (linear in K)")


DUMP_BUDGET_BYTES = 64_000_000


def write_outputs(out_dir: str, arrays) -> None:
    """--dump-outputs: ``arrays`` (name -> tensor / array, what the last timed step returned) as ``out_dir/<name>.npy``,
    floats as float32 / float64, integers as float64 (exact).  Arrays that do not fit the 64 MB budget left by the smaller
    ones keep a fixed, seeded sample of rows along their longest axis; ``<name>_sample_index.npy`` then holds those rows."""
    arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    arrays = {k: (v if v.dtype in (np.float32, np.float64) else v.astype(np.float64)) for k, v in arrays.items()}
    os.makedirs(out_dir, exist_ok=True)
    left = DUMP_BUDGET_BYTES - 2 * 4096 * len(arrays)          # room for the .npy headers of up to two files per array
    for i, (name, a) in enumerate(sorted(arrays.items(), key=lambda kv: kv[1].nbytes)):
        share = left // (len(arrays) - i)
        if a.nbytes > share:
            axis = int(np.argmax(a.shape))
            keep = max(1, share // (a.nbytes // a.shape[axis] + 8))           # rows of the sample + their float64 index
            idx = np.sort(np.random.default_rng(0).choice(a.shape[axis], keep, replace=False))
            a = np.take(a, idx, axis=axis)
            np.save(os.path.join(out_dir, f"{name}_sample_index.npy"), idx.astype(np.float64))
            left -= idx.size * 8
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(a))
        left -= a.nbytes


def detect_outputs(res) -> dict:
    """The caller's view of one detect step: rows [0, count) of every image; the rows past an image's count are stale buffer
    contents (never cleared) and are written as zeros, so that two runs compare equal where their results do."""
    n = res["count"].to(torch.int64).clamp(min=0)
    out = {"count": res["count"]}
    for k in ("bboxes", "scores", "labels", "anchors", "embeddings"):
        if k in res:
            v = res[k]
            live = torch.arange(v.shape[1], device=v.device)[None, :] < n[:, None]
            out[k] = torch.where(live.view(*live.shape, *([1] * (v.dim() - 2))), v, torch.zeros((), dtype=v.dtype, device=v.device))
    return out


def launch_ranks(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, rendezvous on
    127.0.0.1) and pass their output through — rank 0 prints the one JSON line, everything else goes to stderr."""
    import socket
    import subprocess
    share = os.environ.get("WEDETECT_BENCH_SHARE_GPU") == "1"
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < n and not share:
        print(f"bench.py: --gpus {n} asked but {have} HIP device(s) visible; refusing to report a smaller job as n_gpus={n} "
              f"(WEDETECT_BENCH_SHARE_GPU=1 WEDETECT_BENCH_BACKEND=gloo is the single-GPU dry run)", file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    env = dict(os.environ, WEDETECT_BENCH_LAUNCHED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: what RCCL needs on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, usable_cores() // n)))
    return subprocess.call(cmd, env=env)


def claim_stdout():
    """fd 1 carries the ONE JSON line and nothing else.  RCCL writes its version banner and its warnings to stdout, from its own
    threads: beside the line they break the driver's parse, and since the line is longer than PIPE_BUF a write of theirs can land
    in the MIDDLE of it (seen on the one-rank RCCL run of the GPU suite).  So the process's fd 1 is pointed at stderr for everybody
    and the line goes out through a private duplicate of the original."""
    sys.stdout.flush()
    keep = os.dup(1)
    os.dup2(2, 1)
    return os.fdopen(keep, "w")


def main():
    args = parse()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE {world}: the job must have exactly the asked number of ranks")
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    json_out = claim_stdout()
    # dry-run hooks for a single-GPU box: WEDETECT_BENCH_SHARE_GPU=1 puts every rank on device 0 and
    # WEDETECT_BENCH_BACKEND=gloo replaces RCCL (which refuses two ranks on one device)
    if os.environ.get("WEDETECT_BENCH_SHARE_GPU") == "1":
        local = 0
    torch.cuda.set_device(local)
    dist = None
    from wedetect_amd.parallel import PhaseWatchdog
    # every rank carries its own progress deadline: a rank that makes no progress for WEDETECT_BENCH_TIMEOUT seconds
    # (default 300) prints "rank r: stuck in <phase>" and exits non-zero, which makes the launcher fail the whole run —
    # a hung rank names itself instead of leaving seven others waiting in a collective forever
    dog = PhaseWatchdog(rank, float(os.environ.get("WEDETECT_BENCH_TIMEOUT", "300")))
    dog.phase("process-group initialisation")
    # WEDETECT_BENCH_FORCE_DIST=1: join a process group even as the only rank — the one way to run the step's collectives
    # (region all-gathers, closing all-reduces, barriers) on RCCL itself on a one-GPU box (tests/test_gpu_entry.py)
    dist_on = world > 1 or os.environ.get("WEDETECT_BENCH_FORCE_DIST") == "1"
    if dist_on:
        import datetime
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        # the image exports NCCL_DEBUG=VERSION, which makes RCCL print a version banner on STDOUT
        # (next to the one JSON line this script owes the driver): keep warnings, drop the banner
        if os.environ.get("NCCL_DEBUG", "").upper() == "VERSION":
            os.environ["NCCL_DEBUG"] = "WARN"
        backend = os.environ.get("WEDETECT_BENCH_BACKEND", "nccl")
        pg_kw = dict(backend=backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=dog.timeout_s))
        if backend == "nccl":
            # bind the communicator to THIS rank's device up front: barrier() otherwise guesses the device from the current
            # context (the warning in GPUTEST_r04) and a wrong guess hangs on a multi-GPU node
            pg_kw["device_id"] = torch.device("cuda", local)
        dist.init_process_group(**pg_kw)

    from wedetect_amd import lib as L
    from wedetect_amd import weights as W
    from wedetect_amd.engine import ImageTower
    from wedetect_amd.pack import pack
    from wedetect_amd.parallel import RegionGatherer

    B, S, K = args.batch, args.size, args.classes
    if args.mode == "retrieval":
        dog.phase("retrieval leg")
        r = retrieval_leg(L, B, args.regions, K, rank, world, args.steps, args.warmup, dist)
        dt = r["dt"]
        ranks_seen, backend_name = 1, None
        if dist is not None:
            dog.phase("closing collectives")
            t = torch.tensor([dt], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
            one = torch.ones(1, dtype=torch.int32, device="cuda")
            dist.all_reduce(one, op=dist.ReduceOp.SUM)
            ranks_seen, backend_name = int(one.item()), str(dist.get_backend())
        if rank == 0:
            out = {"metric": f"images/s, object retrieval: {args.regions} kept regions per image x {K}-class text bank "
                             "(sigmoid(<e, t> exp(scale) + bias), max over regions; logits never materialised)",
                   "value": round(world * B * args.steps / dt, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps,
                   "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 3), "higher_is_better": True, "scaling": "weak",
                   "vs_baseline": None,
                   "dtype": ("f32-equivalent: fp32 operands carried as fp16 hi+lo pairs, 3 fp16-MFMA passes per product, fp32 accumulate "
                             "(fp16x3), fp32 epilogue" if r["precision"] == "fp16x3" else "f32"),
                   "data": "synthetic",
                   "config": {"workload": f"configs[4]: {B} images per GPU x {args.regions} regions x 768 against a {K}-class bank"
                                          + (f", class-sharded x{world} ({K // world} classes per GPU) + all-gather of regions and score blocks"
                                             if world > 1 else ""),
                              "global_batch": world * B, "per_gpu_batch": B, "regions_per_image": args.regions, "classes": K,
                              "parallelism": f"image-shard x{world} + class-shard x{world}" if world > 1 else "one GPU, whole bank",
                              "precision": r["precision"], "fp16x3_range_guard_tripped": r["tripped"], "score_checksum": r["checksum"]},
                   "roofline": r["roofline"]}
            if dist_on:
                out["ranks_seen"], out["collective_backend"] = ranks_seen, backend_name
            if args.dump_outputs:
                write_outputs(args.dump_outputs, {"scores": r["scores"]})
            if args.full and world == 1 and not args.no_cpu_baseline:
                dog.phase("cpu baseline")
                out["cpu_baseline"] = retrieval_cpu_baseline(args.regions, K)
            print(json.dumps(out), file=json_out, flush=True)
        if dist is not None:
            dog.phase("final barrier")
            dist.barrier()
            dist.destroy_process_group()
        dog.stop()
        return
    tower = ImageTower(args.arch, pack(W.make_state_dict(args.arch), args.arch), B, S, S, max_classes=K,
                       precision=args.precision, split_k=args.split_k or None)
    split = tower.precision == "fp16x3"
    images = torch.from_numpy(W.make_images(B, S, S, seed=1234 + rank)).cuda()
    text = torch.from_numpy(W.make_text_bank(K)).cuda()
    meta = tower.identity_meta()
    uni = args.mode == "uni"
    if not uni:
        meta[:, 7] = 1.0                    # mmdet order: rescale before NMS
    full = args.full
    timer = GemmTimer(L)
    if full:
        timer.install()                     # per-launch stamps on the last timed steps: --full only (a plain run times bare steps)

    gatherer = RegionGatherer(timeout_s=dog.timeout_s) if dist_on else None
    lvl_scale = torch.tensor(tower.lvl_logit_scale, dtype=torch.float32, device="cuda")
    lvl_bias = torch.tensor(tower.lvl_bias, dtype=torch.float32, device="cuda")
    image_ids = torch.arange(rank * B, (rank + 1) * B, dtype=torch.int64, device="cuda")
    stall = []                                  # (event before, event after) around the gather hand-over of a step

    import contextlib
    overlap = not args.no_overlap_post

    def step(measure_stall=False):
        # overlap_post: top-k / NMS of this step on the tower's second stream, beside the next step's backbone (all of it
        # still inside the timed bracket: the closing torch.cuda.synchronize() drains both streams)
        res = tower.detect(images, text, meta, normalize_text=not uni, score_thr=0.0 if uni else 0.001,
                           with_embed=True, overlap_post=overlap)
        if gatherer is None:
            return res
        with (torch.cuda.stream(tower.post_stream) if overlap else contextlib.nullcontext()):
            # the exchange of this batch's kept regions (embeddings + per-region scale / bias + counts + image ids:
            # the four lists of extract_embedding.py:1753-1756) runs behind the next batch's kernels
            lvl = tower.level_of(res["anchors"])
            if measure_stall:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            gatherer.submit(res["embeddings"], res["count"], scales=lvl_scale[lvl], bias=lvl_bias[lvl], image_ids=image_ids)
            if measure_stall:
                e1.record()
                stall.append((e0, e1))
        return res

    def sync():
        if gatherer is not None:
            gatherer.collect()               # every gather started inside the bracket completes inside it
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    dog.phase("calibration + warm-up")
    if not args.no_calibrate:
        tower.calibrate(images)             # as the detectors do on a tower's first batch (untimed; all scales 1 here)
    timer.mode = "count"
    for _ in range(args.warmup):
        step()
    sync()
    dog.phase("timed steps")
    # per-launch kernel timing covers the LAST n_inst steps of the timed region only: stamping every launch costs the
    # step ~1.2 ms (2.4 %: scripts/step_timer_overhead.py), so the headline would otherwise measure its own probe
    n_inst = min(args.steps, 1 if args.steps < 4 else 2)
    if full:
        timer.prepare(timer.count // max(1, args.warmup) * n_inst)
    timer.mode = "off"
    clock = ClockSampler(local) if full else None
    if clock is not None:
        clock.start()
    t0 = time.perf_counter()
    for i in range(args.steps):
        if full and i == args.steps - n_inst:
            timer.mode = "time"
        res = step(measure_stall=dist_on)
    sync()
    dt = time.perf_counter() - t0
    clk = clock.stop() if clock is not None else None
    timer.mode = "off"
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, detect_outputs(res))      # before the serial leg of --full reuses the buffers
    per_rank = None
    ranks_seen, backend_name = 1, None
    dog.phase("closing collectives")
    if dist is not None:
        own = dict(rank=rank, ms_per_step=round(1e3 * dt / args.steps, 3),
                   gather_handover_ms_per_step=round(sum(a.elapsed_time(b) for a, b in stall) / max(1, len(stall)), 3))
        per_rank = [None] * world
        dist.all_gather_object(per_rank, own)
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        one = torch.ones(1, dtype=torch.int32, device="cuda")    # how many ranks the collective library actually joined
        dist.all_reduce(one, op=dist.ReduceOp.SUM)
        ranks_seen, backend_name = int(one.item()), str(dist.get_backend())
    kept = int(res["count"].sum().item())
    overflow = bool((res["count"] < 0).any().item()) or bool(tower.range_flags.any().item())     # fp16x3 range guards

    # Round 6: in the timed region the backbone runs as image chains on two streams and the neck / head of step i beside the
    # backbone of step i + 1 (engine.ImageTower: bb_chains, pipe_neck): a launch then shares the chip with launches of other
    # streams and its begin-to-end time is no longer its own.  The per-kernel figures of the line (roofline, gemm_kernels,
    # sim_gemm) therefore come from a SERIAL LEG — the same step, same kernels, one launch at a time on one stream (DAG lanes of
    # the neck aside, as in rounds 1-5), two warm-ups + n_inst instrumented steps right after the timed region — and the timed
    # region's own stamps are kept beside them (roofline.timed_region).
    concurrent = overlap and (tower._n_chains() > 1 or tower._pipe_neck_on())
    timed_summ = None
    if full and concurrent:
        dog.phase("serial leg (per-kernel timing)")
        timed_summ = timer.summary(busy=True) if rank == 0 else None
        saved_modes = (tower.bb_chains, tower.pipe_neck, tower.force_tile_forms)
        tower.bb_chains, tower.pipe_neck, tower.force_tile_forms = "1", "0", True      # the kernel forms of the pipelined step
        for _ in range(2):
            step()
        sync()
        timer.rec.clear()
        timer.prepare(timer.count // max(1, args.warmup) * n_inst)
        timer.mode = "time"
        for _ in range(n_inst):
            step()
        sync()
        timer.mode = "off"
        tower.bb_chains, tower.pipe_neck, tower.force_tile_forms = saved_modes

    if rank == 0:
        if full:
            summ = timer.summary()
            dom_tag = max(summ, key=lambda k: summ[k]["flops_total"])
            dom = summ[dom_tag]
            flops_img = sum(v["flops_total"] for v in summ.values()) / (n_inst * B)
            dom_split = dom_tag.startswith("fp16x3")
            # fp16x3 issues three fp16 MFMA passes per fp32-accurate product: the roof for ALGORITHMIC
            # flops is the fp16 dense peak / 3; the fraction of the raw fp16 peak is reported beside it.
            dom_peak = round(F16_MFMA_PEAK_TFLOPS / SPLIT_PASSES, 1) if dom_split else F32_MFMA_PEAK_TFLOPS
            dom_fn = ("split_gemm_p8" if "/p8" in dom_tag else "split_gemm_p4" if "/p4" in dom_tag else "split_gemm_glds" if "glds" in dom_tag
                      else "split_gemm_pingpong" if "pingpong" in dom_tag else "split_gemm")
            dom_kernel = (f"{dom_fn}_kernel<{dom_tag}> (3 x v_mfma_f32_32x32x16_f16 per product)" if dom_split
                          else f"conv_gemm_kernel<{dom_tag}> (fp32 MFMA 16x16x4)")
            traffic, traffic_src = (measured_traffic(dom_tag) if (B, S, K, args.arch, args.mode) == (32, 640, 80, "base", "detect")
                                    else (None, None))
        out = {
            "metric": f"images/s at {S}x{S} (WeDetect-{args.arch.capitalize()} image tower + {K}-class similarity + top-k/NMS)",
            "value": round(world * B * args.steps / dt, 3),
            "unit": "images/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": ("f32-equivalent: fp32 operands carried as fp16 hi+lo pairs, 3 fp16-MFMA passes per product, fp32 "
                      "accumulate (fp16x3); similarity GEMM, dwconv, LN, post-process native f32") if split else "f32",
            "data": "synthetic",
            "config": {"workload": f"WeDetect-{args.arch.capitalize()}, batch {B}x{S}x{S} per GPU, {K}-class similarity, "
                                   f"thr {0.0 if uni else 0.001} / nms_pre 30000 / NMS 0.7 / 300 per image, mode {args.mode}",
                       "global_batch": world * B, "per_gpu_batch": B, "image": [S, S], "classes": K,
                       "parallelism": f"image-shard x{world}" + (" + all-gather of kept-region embeddings" if world > 1 else ""),
                       "precision": tower.precision,
                       "pipelining": (("neck + head + similarity of step i on the tower's nh stream and its top-k / NMS on the post stream beside "
                                       "the backbone of step i + 1" if tower._pipe_neck_on() else
                                       "top-k / NMS of step i on a second stream beside the backbone of step i + 1")
                                      + (f"; two backbones in flight (steps alternate between two backbone streams)" if tower._pipe_neck_on() and tower._bb_depth() == 2
                                         else f"; backbone as {tower._n_chains()} image chain(s)")
                                      + " (same kernels, bit-identical results; every step completes inside the timed bracket); "
                                        "--no-overlap-post issues a step's kernels in line"
                                      if overlap else "none: every kernel of a step on one stream"),
                       **({"precision_evidence": "error vs a float64 run of the same network (oracle, Base@128): embeddings "
                           "fp32 8.5e-6 / fp16x3 9.5e-6, scores 8.0e-7 / 9.2e-7 (tests/probe_split_precision.py); on device the "
                           "fp16x3 step is within 5e-5 (embeddings) / 1e-5 (scores) of the fp32 step at this size "
                           "(tests/test_gpu_precision.py); --precision fp32 runs native fp32 MFMA"} if split else {}),
                       "kept_regions_last_step_rank0": kept, "fp16x3_range_guard_tripped": overflow,
                       "fp16x3_trips": int(tower.fp16x3_trips) + int(overflow),      # ImageTower's counter (checked_counts) + this run's raw flags
                       **({"gemm_gflop_per_image": round(flops_img / 1e9, 2)} if full else {})},
            **({"roofline": {"kernel": dom_kernel, "bound": "mfma",
                         "achieved": round(dom["tflops"], 2), "peak": dom_peak, "unit": "TFLOP/s",
                         "frac": round(dom["tflops"] / dom_peak, 4),
                         **({"effective_mhz": clk["mean_mhz"], "effective_mhz_min_max": [clk["min_mhz"], clk["max_mhz"]],
                             "clock_samples": clk["samples"], "clock_source": clk["source"], "peak_quoted_at_mhz": PEAK_CLOCK_MHZ,
                             "frac_at_effective_clock": round(dom["tflops"] / dom_peak * PEAK_CLOCK_MHZ / clk["mean_mhz"], 4),
                             "clock_note": "shader clock sampled every 10 ms from sysfs during the timed steps: the chip is "
                                           "power-limited in this step; frac stays against the spec peak"} if clk else
                            {"effective_mhz": None}),
                         **({"peak_note": f"fp16 dense MFMA peak {F16_MFMA_PEAK_TFLOPS} / {SPLIT_PASSES} passes per product",
                             "mfma_issued_tflops": round(SPLIT_PASSES * dom["tflops"], 1),
                             "frac_of_fp16_peak": round(SPLIT_PASSES * dom["tflops"] / F16_MFMA_PEAK_TFLOPS, 4)} if dom_split else {}),
                         "traffic": traffic, "traffic_provenance": traffic_src,
                         "traffic_unit": "HBM bytes per launch (PMC, separate rocprofv3 passes; see traffic_provenance)",
                         **({"power_limited_ceiling": power_ceiling()} if dom_split else {}),
                         "timing": "HIP events stamped by each kernel's own dispatch (hipExtLaunchKernelGGL via "
                                   "wd_time_next_gemm) on the launch stream, every GEMM launch of "
                                   + (f"the serial leg's {n_inst} instrumented steps (measured_in)" if concurrent else
                                      f"the last {n_inst} of the {args.steps} timed steps (stamping all steps would slow the step it measures by 2.4 %)"),
                         "algorithmic_bytes_per_launch": round(dom["bytes_total"] / dom["launches"]),
                         "launches_per_step": dom["launches"] // n_inst, "avg_launch_us": round(dom["avg_us"], 2),
                         "algorithmic_gflop_per_launch": round(dom["flops_total"] / dom["launches"] / 1e9, 3),
                         **({"measured_in": f"serial leg: {n_inst} instrumented steps after two warm-ups, right after the timed region, "
                                            "with WEDETECT_BB_CHAINS=1 WEDETECT_PIPE_NECK=0 WEDETECT_FORCE_TILE=1 semantics (one backbone chain, neck / head in line, the tile forms the pipelined backbone runs) — "
                                            "in the timed region launches of several streams share the chip (timed_region below)",
                             "timed_region": timed_region_record(timed_summ, dom_tag, dom_peak, n_inst, tower)} if concurrent else {})},
            "gemm_kernels": {k: {"launches_per_step": v["launches"] // n_inst, "avg_us": round(v["avg_us"], 2),
                                 "tflops": round(v["tflops"], 2)} for k, v in sorted(summ.items())}} if full else {}),
        }
        if per_rank is not None:
            out["per_rank"] = per_rank
            out["ranks_seen"] = ranks_seen          # all_reduce(1) over the job's process group: the collective library saw this many
            out["collective_backend"] = backend_name
        if full:
            simrec = sim_record(summ, L, B * tower.ntot, K)
            if simrec is not None:
                out["sim_gemm"] = simrec
                if simrec["dtype"] == "fp16x3":                   # a bank of >= 256 rows: keep the fp32-MFMA figure beside it
                    out["sim_gemm"]["fp32_kernel"] = fp32_sim_reference(tower, L, text, not uni)
            dog.phase("side legs (fp32 reference, host-fed, other configurations, cpu baseline)")
            dog.timeout_s = max(dog.timeout_s, 900.0)
            if world == 1 and split and not args.no_fp32_reference:
                # the same workload with native fp32 MFMA arithmetic, measured in this run (same images, weights, bank)
                out["fp32_mode"] = fp32_reference_run(args, tower, images, text, meta, uni)
            if world == 1 and not args.no_host_fed:
                out["host_fed"] = host_fed_run(tower, images, text, meta, uni, min(args.steps, 20))
            if (world == 1 and split and not args.no_other_configs
                    and (B, S, K, args.arch, args.mode) == (32, 640, 80, "base", "detect")):
                # configs[2], [3] (one rank's share) and [4] (per-GPU form, whole bank) in the driver's one line: twenty timed steps (configs[4]: five)
                # each after two warm-ups, same protocol as the headline
                other = {}
                other["configs[2] large_b16_k1203"] = detect_leg(timer, L, "large", 16, 1203, uni=False)
                other["configs[3] base_uni_b32_k256 (one rank's step; the exchange is the --gpus N path)"] = detect_leg(timer, L, "base", 32, 256, uni=True)
                r = retrieval_leg(L, 32, 300, 1_000_000, 0, 1, steps=5, warmup=2)
                other["configs[4] retrieval_1m_classes (per-GPU form: 32 images x 300 regions, whole bank)"] = {
                    "value": round(32 * 5 / r["dt"], 3), "unit": "images/s", "ms_per_step": round(1e3 * r["dt"] / 5, 3), "steps": 5, "warmup": 2,
                    "precision": r["precision"], "fp16x3_range_guard_tripped": r["tripped"], "roofline": r["roofline"]}
                out["other_configs"] = other
            if world == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(args.arch, S, K, args.cpu_runs)
        print(json.dumps(out), file=json_out, flush=True)
    if dist is not None:
        dog.phase("final barrier")
        dist.barrier()
        dist.destroy_process_group()
    dog.stop()


if __name__ == "__main__":
    main()
