"""Dataset-loop throughput of test.py, serial loader against streamed loader, in one process.

    python scripts/stream_bench.py [--n 2048] [--batch 32] [--size base] [--rounds 3] [--small 1,8] [--bench-value X]

Writes N seeded JPEGs of COCO-like sizes (smooth low-frequency content plus a little noise, so that the files are about
photograph-sized; white noise decodes atypically slowly) into a temporary directory, builds the detector with synthetic
weights and an 80-class bank, warms every tower shape both ways, then runs test.py's two loops (``predict_shard`` — the
loop as it was before the streamed loader, unchanged — and ``predict_shard_stream``) alternately, serial / stream / serial /
stream ..., each timed by the wall clock around a full drain.  The spread of a leg is taken over its repetitions.  Also
measured: the decode-only rate of the worker pool (the same threads decoding the same files, nothing else) and the
``stats`` counters of the streamed legs.  ``--small`` repeats the comparison at other batch sizes on a subset of the files.
``--bench-value``: the same machine's plain ``python bench.py`` images/s, for the share line.  Prints everything and writes
profiles/stream_loader.txt.
"""
import argparse
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(640, 480), (480, 640), (640, 427), (500, 375), (333, 500), (640, 426), (427, 640), (612, 612), (640, 360), (500, 333)]


def write_images(folder: str, n: int, seed: int = 2026, workers: int = 8):
    from PIL import Image

    def one(k):
        rng = np.random.default_rng([seed, k])
        w, h = SIZES[k % len(SIZES)]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        chans = []
        for c in range(3):
            a = np.zeros((h, w), np.float32)
            for _ in range(3):                            # a few low-frequency waves per channel
                fx, fy, ph = rng.uniform(0.003, 0.04), rng.uniform(0.003, 0.04), rng.uniform(0, 6.28)
                a += rng.uniform(20, 45) * np.sin(fx * xx + ph) * np.cos(fy * yy + ph * 0.7)
            chans.append(127 + a + rng.normal(0, 6, (h, w)).astype(np.float32))
        path = os.path.join(folder, f"{k:06d}.jpg")
        Image.fromarray(np.clip(np.stack(chans, -1), 0, 255).astype(np.uint8)).save(path, quality=90)
        return path
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(one, range(n)))


class FileList:
    """What test.py's loops need of a dataset: ``get_data_info`` and ``pipeline``."""

    def __init__(self, paths, texts, pipeline):
        from wedetect_amd.pipeline import Compose
        self.paths, self.texts, self.pipeline = paths, texts, Compose(pipeline)

    def __len__(self):
        return len(self.paths)

    def get_data_info(self, i):
        return dict(img_id=i, img_path=self.paths[i], texts=self.texts)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", default="base")
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", default="1,8", help="other batch sizes to compare, on --small-n files")
    ap.add_argument("--small-n", type=int, default=256)
    ap.add_argument("--decode-workers", type=int, default=None)
    ap.add_argument("--bench-value", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_loader.txt"))
    args = ap.parse_args(argv)

    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("wd_test_entry", os.path.join(ROOT, "test.py"))   # the repository's test.py, not the stdlib package
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    from wedetect_amd import weights as W
    from wedetect_amd.cfgfile import Config
    from wedetect_amd.detector import YOLOWorldDetector
    from wedetect_amd.stream import _load_rgb, decode_pool_size

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    workers = decode_pool_size(args.decode_workers)
    cfg = Config.fromfile(os.path.join(ROOT, "config", f"wedetect_{args.size}.py"))
    pipeline = [p.to_dict() if hasattr(p, "to_dict") else dict(p) for p in cfg.test_dataloader.dataset.pipeline]
    names = [f"class {k}" for k in range(args.classes)]
    texts = [[n] for n in names]
    with tempfile.TemporaryDirectory(prefix="wd_stream_bench_") as folder:
        t0 = time.perf_counter()
        paths = write_images(folder, args.n, workers=workers)
        mb = sum(os.path.getsize(p) for p in paths) / 1e6
        say(f"# {args.n} JPEGs, {mb / args.n * 1e3:.0f} kB mean, written in {time.perf_counter() - t0:.1f} s; sizes {SIZES}")
        model = YOLOWorldDetector(args.size, max_classes=args.classes)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict(args.size).items()})
        model.cuda().eval()
        model.set_text_embeddings(torch.from_numpy(W.make_text_bank(args.classes)).cuda(), texts)
        say(f"# {torch.cuda.get_device_name(0)}; model {args.size}, {args.classes} classes, precision {model._h.precision or 'default'}, "
            f"decode workers {workers}")

        # decode-only rate of the worker pool: the same threads, the same files, nothing else
        def decode_rate(files):
            t = time.perf_counter()
            with ThreadPoolExecutor(max_workers=workers) as ex:
                for a in ex.map(lambda p: _load_rgb(p, True), files):
                    pass
            return len(files) / (time.perf_counter() - t)
        decode_rate(paths[:256])
        rates = [decode_rate(paths) for _ in range(2)]
        dec = max(rates)
        say(f"decode-only rate of the pool ({workers} threads, {args.n} files): {rates[0]:.0f} / {rates[1]:.0f} images/s")

        def leg(kind, ds, bs):
            stats = {}
            torch.cuda.synchronize()
            t = time.perf_counter()
            if kind == "serial":
                preds = T.predict_shard(model, ds, range(len(ds)), bs)
            else:
                preds = T.predict_shard_stream(model, ds, range(len(ds)), bs, args.decode_workers, stats)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            assert len(preds) == len(ds)
            return len(ds) / dt, stats, preds

        results = {}
        for bs, files in [(args.batch, paths)] + [(int(b), paths[:args.small_n]) for b in args.small.split(",") if b.strip()]:
            ds = FileList(files, texts, pipeline)
            warm = FileList(files[:2 * bs + (len(files) % bs)], texts, pipeline)        # both tower shapes, both loops
            leg("serial", warm, bs)
            leg("stream", warm, bs)
            per = {"serial": [], "stream": []}
            last = {}
            for r in range(args.rounds):
                for kind in ("serial", "stream"):
                    v, stats, preds = leg(kind, ds, bs)
                    per[kind].append(v)
                    last[kind] = preds
                    extra = ""
                    if kind == "stream":
                        extra = (f"  feed launches/batch max {stats['feed_launches_max']}, H2D/batch max {stats['h2d_copies_max']}, "
                                 f"D2H/batch max {stats['d2h_copies_max']}, in flight max {stats['max_in_flight']}, batches {stats['batches']}, "
                                 f"trips {stats['trips']}, in-line {stats['inline_batches']}, arena grows {stats['arena_grows']}")
                    say(f"batch {bs:3d} round {r} {kind:6s}: {v:8.1f} images/s{extra}")
            same = all(torch.equal(a["pred_instances"][k], b["pred_instances"][k]) for a, b in zip(last["serial"], last["stream"])
                       for k in ("bboxes", "scores", "labels"))
            s, t = np.asarray(per["serial"]), np.asarray(per["stream"])
            spread = max(s.max() - s.min(), t.max() - t.min())
            results[bs] = (s, t, spread)
            say(f"batch {bs:3d}: serial {s.mean():.1f} (min {s.min():.1f}, max {s.max():.1f}), stream {t.mean():.1f} (min {t.min():.1f}, "
                f"max {t.max():.1f}) images/s over {len(files)} files; ratio {t.mean() / s.mean():.2f}x; spread {spread:.1f}; "
                f"stream - serial = {t.mean() - s.mean():.1f}; predictions identical: {same}")
        s, t, _ = results[args.batch]
        bound = [("decode-only rate", dec)] + ([("bench.py plain", args.bench_value)] if args.bench_value else [])
        name, lim = min(bound, key=lambda kv: kv[1])
        say(f"streamed rate at batch {args.batch}: {t.mean():.1f} images/s = {100 * t.mean() / lim:.0f} % of min("
            + ", ".join(f"{k} {v:.0f}" for k, v in bound) + f"); {name} binds")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
