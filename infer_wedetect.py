"""Open-vocabulary detection demo on the MI355X path — command-line compatible with the reference's
``infer_wedetect.py`` (its flags: infer_wedetect.py:59-98; its flow: 150-195):

    python infer_wedetect.py --config config/wedetect_base.py --checkpoint ckpt.pth \
        --image demo.jpg --text '鞋,床' --threshold 0.3 --device cuda:0

config -> ``init_detector`` -> ``Compose(cfg.test_pipeline)`` -> texts ``[[t], ...] + [[' ']]`` (the blank class the
reference appends) -> ``model.reparameterize(texts)`` -> per image: pipeline, ``test_step``, score filter, top-k,
annotated copy in ``--output-dir``.  Everything numeric runs through libwedetect_hip.so.

Additions (absent from the reference, all optional): ``--text-bank FILE`` loads a precomputed ``[K + 1, 768]`` class
bank (``.npy`` / ``.pt``; rows for the K prompts then the blank) instead of running the text tower — for hosts without
the XLM-R tokenizer files; ``--precision {fp32,fp16x3}``; ``--dump-json`` also writes the kept detections per image;
``--tile N`` (default 0 = off) runs every image through ``YOLOWorldDetector.predict_tiled`` — overlapping N x N crops
(``--tile-overlap``, ``--tile-batch`` tiles per step, ``--edge-margin``) plus one overview of the whole image
(``--no-overview``), merged on the device — before the same ``--threshold`` / ``--topk`` filter;
``--exemplar-image PATH --exemplar-boxes "x1,y1,x2,y2:name;..."`` (off by default) builds classes from example boxes of one
image instead of text (``YOLOWorldDetector.exemplar_bank``; a name that repeats is ONE class with several examples,
``--anchors-per-box`` anchors are pooled per box, ``--save-bank OUT.pt`` keeps the rows) — with ``--text`` the exemplar classes
are appended after the text classes, without it they are the whole bank; ``--tune-steps N`` (default 0 = off; ``--tune-lr``)
then refines the exemplar rows on the same boxes by N Adam steps with both towers frozen
(``YOLOWorldDetector.tune_bank``) before detection: with ``--text`` the text rows are frozen and serve as negatives, and
``--save-bank`` keeps the tuned rows.
"""
import argparse
import json
import os
import os.path as osp
import random
import sys

import numpy as np
import torch

from wedetect_amd.apis import inference_detector, init_detector
from wedetect_amd.cfgfile import Config, DictAction
from wedetect_amd.pipeline import Compose


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Demo")
    parser.add_argument("--config", help="test config file path")
    parser.add_argument("--checkpoint", help="checkpoint file")
    parser.add_argument("--image", help="image path, include image file or dir.")
    parser.add_argument("--text", help="text prompts, including categories separated by a comma or a txt file with "
                                       "each line as a prompt.")
    parser.add_argument("--topk", default=100, type=int, help="keep topk predictions.")
    parser.add_argument("--threshold", default=0.05, type=float, help="confidence score threshold for predictions.")
    parser.add_argument("--device", default="cuda:0", help="device used for inference.")
    parser.add_argument("--show", action="store_true", help="show the detection results.")
    parser.add_argument("--amp", action="store_true", help="accepted for compatibility: the device path always "
                                                           "computes at fp32-equivalent accuracy")
    parser.add_argument("--output-dir", default="demo_outputs", help="the directory to save outputs")
    parser.add_argument("--cfg-options", nargs="+", action=DictAction,
                        help="override some settings in the used config, the key-value pair in xxx=yyy format will be "
                             "merged into config file.")
    parser.add_argument("--text-bank", default=None, help="precomputed [K+1, 768] class embeddings (.npy / .pt)")
    parser.add_argument("--precision", default=None, choices=["fp32", "fp16x3"])
    parser.add_argument("--dump-json", action="store_true", help="write <image>.json with the kept detections")
    parser.add_argument("--tile", default=0, type=int, help="tiled inference on overlapping N x N crops (a multiple of 32); 0 = off")
    parser.add_argument("--tile-overlap", default=0.2, type=float, help="overlap of neighbouring tiles, 0 .. 0.5 of the tile")
    parser.add_argument("--tile-batch", default=32, type=int, help="tiles per tower step")
    parser.add_argument("--no-overview", action="store_true", help="no letterboxed overview of the whole image beside the crops")
    parser.add_argument("--edge-margin", default=2.0, type=float,
                        help="drop rows closer than this many pixels to an interior side of their crop")
    parser.add_argument("--best-class", action="store_true",
                        help="single-label detection: one label per box, the best name of the bank (the reference's multi_label=False)")
    parser.add_argument("--agnostic-nms", action="store_true",
                        help="with --best-class: NMS across labels (mmcv batched_nms class_agnostic=True)")
    parser.add_argument("--sparse-scores", action="store_true",
                        help="multi-label detection without the [B, 8400, K] score tensor: candidates above the threshold as "
                             "per-image lists (same results; a list that overflows falls back to the dense step)")
    parser.add_argument("--sparse-cap", default=65536, type=int, help="with --sparse-scores: list entries per image, rounded up to a power of two and to at least the top-k "
                             "capacity of test_cfg.nms_pre (32768 for 30000); up to 2^20")
    parser.add_argument("--top-names", default=0, type=int,
                        help="with --best-class: keep the N (1..8) best names of every box; --dump-json then writes them as "
                             "\"names\": [[name, score], ...] per detection (the drawn label stays the first)")
    parser.add_argument("--prompt-groups", action="store_true",
                        help="score every class as the best of several names: inside --text, '/' separates the names of one class "
                             "(\"person/man/woman,dog/puppy\"); --text-bank then holds one row per NAME plus the blank class")
    parser.add_argument("--exemplar-image", default=None, help="image that holds the example boxes of --exemplar-boxes")
    parser.add_argument("--exemplar-boxes", default=None,
                        help="example boxes in pixels of --exemplar-image, \"x1,y1,x2,y2:name;...\"; a name that repeats is one class "
                             "with several examples; the classes follow the --text classes")
    parser.add_argument("--anchors-per-box", default=4, type=int, help="with --exemplar-boxes: anchors pooled per example box, 1..8")
    parser.add_argument("--save-bank", default=None, help="with --exemplar-boxes: write the [C, 768] exemplar rows to this .pt file")
    parser.add_argument("--tune-steps", default=0, type=int,
                        help="with --exemplar-boxes: refine the exemplar rows on the same boxes by this many Adam steps, towers "
                             "frozen (--text rows are frozen negatives); 0 = off")
    parser.add_argument("--tune-lr", default=1e-2, type=float, help="with --tune-steps: Adam's learning rate (a parameter, not a tuned value)")
    parser.add_argument("--track", action="store_true",
                        help="treat the images of an --image directory as ONE video in name order: detections keep their ids from "
                             "frame to frame (associated on the device from boxes and region embeddings); --dump-json gains "
                             "\"track_id\" per detection (0 = no track)")
    parser.add_argument("--track-batch", default=8, type=int, help="with --track: consecutive frames per tower step")
    parser.add_argument("--track-high", default=0.5, type=float, help="with --track: first round takes scores >= this")
    parser.add_argument("--track-low", default=0.1, type=float, help="with --track: second round takes scores from this up to --track-high")
    parser.add_argument("--track-new", default=0.6, type=float, help="with --track: an unmatched detection starts a track from this score")
    parser.add_argument("--track-match", default=0.3, type=float, help="with --track: least similarity of a first-round match")
    parser.add_argument("--track-iou2", default=0.5, type=float, help="with --track: least IoU of a second-round match")
    parser.add_argument("--track-w-iou", default=0.5, type=float, help="with --track: weight of the IoU against the appearance term, 0 .. 1")
    parser.add_argument("--track-max-age", default=30, type=int, help="with --track: frames a track survives unmatched")
    parser.add_argument("--track-labels", action="store_true", help="with --track: a match needs equal labels")
    parser.add_argument("--track-assign", default="greedy", choices=("greedy", "optimal"),
                        help="with --track: how a round associates detections with tracks: the greedy picks, or the "
                             "maximum-weight (Hungarian) matching solved on the device")
    args = parser.parse_args(argv)
    args.exemplars = None
    if not args.track and any(a.startswith("--track-") for a in (sys.argv[1:] if argv is None else argv)):
        parser.exit(2, "infer_wedetect.py: a --track-... option needs --track\n")
    if args.track:
        if args.track_batch < 1:
            parser.exit(2, "infer_wedetect.py: --track-batch takes a count >= 1\n")
        if args.prompt_groups or args.tile > 0:
            parser.exit(2, "infer_wedetect.py: --track is not implemented together with --prompt-groups or --tile\n")
        try:
            track_params(args)
        except ValueError as e:
            parser.exit(2, f"infer_wedetect.py: --track: {e}\n")
    if args.tune_steps < 0 or not 0 < args.tune_lr < float("inf"):
        parser.exit(2, "infer_wedetect.py: --tune-steps takes a count >= 0 and --tune-lr a positive rate\n")
    if args.tune_steps and args.exemplar_boxes is None:
        parser.exit(2, "infer_wedetect.py: --tune-steps needs --exemplar-boxes\n")
    if (args.exemplar_image is None) != (args.exemplar_boxes is None):
        parser.exit(2, "infer_wedetect.py: --exemplar-image and --exemplar-boxes go together\n")
    if args.exemplar_boxes is not None:
        try:
            args.exemplars = parse_exemplar_boxes(args.exemplar_boxes)
        except ValueError as e:
            parser.exit(2, f"infer_wedetect.py: --exemplar-boxes: {e}\n")
        if not 1 <= args.anchors_per_box <= 8:
            parser.exit(2, "infer_wedetect.py: --anchors-per-box takes 1 .. 8\n")
        if args.prompt_groups:
            parser.exit(2, "infer_wedetect.py: --exemplar-boxes is not implemented together with --prompt-groups\n")
    elif args.save_bank is not None:
        parser.exit(2, "infer_wedetect.py: --save-bank needs --exemplar-boxes\n")
    if args.prompt_groups and (args.best_class or args.sparse_scores or args.top_names):
        parser.exit(2, "infer_wedetect.py: --prompt-groups excludes --best-class, --sparse-scores and --top-names\n")
    if args.prompt_groups and args.tile > 0:
        parser.exit(2, "infer_wedetect.py: --prompt-groups is not implemented for tiled inference (--tile)\n")
    if args.top_names and not args.best_class:
        parser.exit(2, "infer_wedetect.py: --top-names needs --best-class\n")
    if not 0 <= args.top_names <= 8:
        parser.exit(2, "infer_wedetect.py: --top-names takes 0 .. 8\n")
    if args.sparse_scores and args.best_class:
        parser.exit(2, "infer_wedetect.py: --sparse-scores (multi-label) and --best-class (single-label) exclude each other\n")
    if args.sparse_scores and args.tile > 0:
        parser.exit(2, "infer_wedetect.py: --sparse-scores is not implemented for tiled inference (--tile)\n")
    if args.agnostic_nms and not args.best_class:
        parser.exit(2, "infer_wedetect.py: --agnostic-nms needs --best-class\n")
    if args.best_class and args.tile > 0:
        parser.exit(2, "infer_wedetect.py: --best-class is not implemented for tiled inference (--tile)\n")
    return args


def track_params(args):
    """The --track-... flags as a ``track.TrackParams`` (ValueError when they contradict each other)."""
    from wedetect_amd.track import TrackParams
    return TrackParams(high_thr=args.track_high, low_thr=args.track_low, new_thr=args.track_new, match_thr=args.track_match,
                       iou2_thr=args.track_iou2, w_iou=args.track_w_iou, max_age=args.track_max_age, match_labels=args.track_labels)


def tracked_detections(model, images, texts, test_pipeline, args):
    """``--track``: the images as one video, ``--track-batch`` frames per ``model.track`` call; yields one host-side
    ``InstanceData`` per image, filtered like ``inference_detector`` (score, top-k), with ``track_ids`` / ``track_hits``."""
    params = track_params(args)
    for i in range(0, len(images), args.track_batch):
        infos = [test_pipeline(dict(img_id=i + k, img_path=p, texts=texts)) for k, p in enumerate(images[i:i + args.track_batch])]
        outs = model.track(torch.stack([d["inputs"] for d in infos]), [d["data_samples"] for d in infos], n_seq=1, track_params=params,
                           assignment=args.track_assign)
        for o in outs:
            pred = o.pred_instances
            pred = pred[pred.scores.float() > args.threshold]
            if len(pred.scores) > args.topk:
                pred = pred[pred.scores.float().topk(args.topk)[1]]
            yield pred.cpu().numpy()


def parse_exemplar_boxes(spec: str):
    """``"x1,y1,x2,y2:name;..."`` -> (class names in order of first appearance, [(box, class index), ...]); ValueError otherwise."""
    names, out = [], []
    for item in [t.strip() for t in spec.split(";") if t.strip()]:
        coords, sep, name = item.partition(":")
        vals = [v.strip() for v in coords.split(",")]
        name = name.strip()
        if not sep or not name or len(vals) != 4:
            raise ValueError(f"{item!r} is not x1,y1,x2,y2:name")
        box = tuple(float(v) for v in vals)
        if not (box[2] > box[0] and box[3] > box[1]):
            raise ValueError(f"{item!r}: the box needs a positive width and height")
        if name not in names:
            names.append(name)
        out.append((box, names.index(name)))
    if not out:
        raise ValueError("no box given")
    return names, out


def read_texts(spec: str, groups: bool = False):
    """infer_wedetect.py:162-167.  ``groups`` (--prompt-groups): '/' separates the names of one class."""
    if spec.endswith(".txt"):
        with open(spec) as f:
            lines = f.readlines()
        items = [t.rstrip("\r\n") for t in lines]
    else:
        items = [t.strip() for t in spec.split(",")]
    if groups:
        return [[n.strip() for n in t.split("/") if n.strip()] or [t] for t in items] + [[" "]]
    return [[t] for t in items] + [[" "]]


def list_images(path: str):
    """infer_wedetect.py:174-180."""
    if not osp.isfile(path):
        return [osp.join(path, img) for img in sorted(os.listdir(path)) if img.endswith(".png") or img.endswith(".jpg")]
    return [path]


def load_bank(path: str) -> torch.Tensor:
    bank = np.load(path) if path.endswith(".npy") else torch.load(path, map_location="cpu")
    if isinstance(bank, dict):
        bank = bank.get("text_embedding", next(iter(bank.values())))
    return torch.as_tensor(np.asarray(bank), dtype=torch.float32)


def visualize(output_file, image_path, bboxes, labels):
    from PIL import Image, ImageDraw, ImageFont
    image = Image.open(image_path).convert("RGB")
    draw = ImageDraw.Draw(image)
    try:
        font = ImageFont.truetype("simsun.ttc", 20)          # the reference's CJK font, when the host has it
    except OSError:
        font = ImageFont.load_default()
    rnd = random.Random(0)
    for box, label in zip(bboxes, labels):
        color = (rnd.randint(0, 255), rnd.randint(0, 255), rnd.randint(0, 255))
        x1, y1, x2, y2 = (float(v) for v in box)
        draw.rectangle([x1, y1, x2, y2], outline=color, width=2)
        draw.rectangle([x1, y1, x1 + len(label) * 20, y1 + 20], fill=color)
        try:
            draw.text((x1 + 2, y1 + 2), label, font=font, fill="white")
        except UnicodeEncodeError:                           # bitmap fallback font without CJK glyphs
            draw.text((x1 + 2, y1 + 2), label.encode("ascii", "replace").decode(), font=font, fill="white")
    image.save(output_file)


def tiled_detections(model, image_path, texts, args):
    """``--tile N``: the image through ``predict_tiled``, then the filter of ``inference_detector`` (score, top-k)."""
    from PIL import Image, ImageOps
    with Image.open(image_path) as im:
        rgb = np.asarray(ImageOps.exif_transpose(im).convert("RGB"))
    pred = model.predict_tiled(rgb, texts, tile=(args.tile, args.tile), overlap=args.tile_overlap, overview=not args.no_overview,
                               tile_batch=args.tile_batch, edge_margin=args.edge_margin).pred_instances
    pred = pred[pred.scores.float() > args.threshold]
    if len(pred.scores) > args.topk:
        pred = pred[pred.scores.float().topk(args.topk)[1]]
    return pred.cpu().numpy()


def main(argv=None, tokenizer=None):
    args = parse_args(argv)
    cfg = Config.fromfile(args.config)
    if args.cfg_options is not None:
        cfg.merge_from_dict(args.cfg_options)
    cfg.work_dir = osp.join("./work_dirs", osp.splitext(osp.basename(args.config))[0])
    if args.best_class:
        cfg.merge_from_dict({"model.best_class": True, "model.agnostic_nms": bool(args.agnostic_nms)})
    if args.top_names:
        cfg.merge_from_dict({"model.top_names": int(args.top_names)})
    if args.sparse_scores:
        cfg.merge_from_dict({"model.sparse_scores": True, "model.sparse_cap": int(args.sparse_cap)})
    if args.prompt_groups:
        cfg.merge_from_dict({"model.prompt_groups": True})
    model = init_detector(cfg, checkpoint=args.checkpoint, device=args.device, palette=["red"], tokenizer=tokenizer,
                          precision=args.precision)
    test_pipeline = Compose(cfg.test_pipeline)
    texts = read_texts(args.text, args.prompt_groups) if (args.text or args.exemplars is None) else []
    if not osp.exists(args.output_dir):
        os.makedirs(args.output_dir)
    images = list_images(args.image)
    if not texts:
        pass                                                 # exemplar classes only
    elif args.text_bank:
        bank = load_bank(args.text_bank)
        n_rows = sum(len(t) for t in texts) if args.prompt_groups else len(texts)
        if bank.shape != (n_rows, 768):
            raise SystemExit(f"--text-bank holds {tuple(bank.shape)}, expected ({n_rows}, 768): one row per prompt "
                             f"plus the blank class")
        model.set_text_embeddings(bank, texts)
    else:
        model.reparameterize(texts)
    if args.exemplars is not None:
        ex_names, ex_list = args.exemplars
        info = test_pipeline(dict(img_id=0, img_path=args.exemplar_image, texts=[[t] for t in ex_names]))
        ex_bank, ex_info = model.exemplar_bank(info["inputs"].unsqueeze(0), [info["data_samples"]], [ex_list], ex_names,
                                               anchors_per_box=args.anchors_per_box)
        print(f"exemplar classes {ex_names}: anchors pooled per class {ex_info['support']}", flush=True)
        bank = torch.cat([model.text_feats.to(ex_bank.device), ex_bank]) if texts else ex_bank
        if args.tune_steps:
            # the exemplar rows learn on the same boxes; the text rows (their blank class included) are frozen negatives
            n_text = bank.shape[0] - ex_bank.shape[0]
            bank, tn = model.tune_bank(info["inputs"].unsqueeze(0), [info["data_samples"]], [[(box, n_text + c) for box, c in ex_list]],
                                       init=bank, steps=args.tune_steps, lr=args.tune_lr, frozen_rows=list(range(n_text)),
                                       anchors_per_box=args.anchors_per_box)
            ex_bank = bank[n_text:]
            print(f"tuned {len(ex_names)} exemplar rows beside {n_text} frozen rows: loss {tn['loss'][0]:.4f} -> {tn['loss'][-1]:.4f} "
                  f"before the last of {args.tune_steps} steps, positives per class {tn['positives'][n_text:]}", flush=True)
        if args.save_bank:
            torch.save(ex_bank.cpu(), args.save_bank)
        texts = texts + [[t] for t in ex_names]              # appended after the text classes (their blank class included)
        model.set_text_embeddings(bank, texts)
    results = []
    tracked = tracked_detections(model, images, texts, test_pipeline, args) if args.track else None
    for n, image_path in enumerate(images):
        if tracked is not None:
            pred = next(tracked)
        elif args.tile > 0:
            pred = tiled_detections(model, image_path, texts, args)
        else:
            pred = inference_detector(model, image_path, texts, test_pipeline, args.topk, args.threshold)
        labels = [f"{texts[c][0]} {s:0.2f}" for c, s in zip(pred["labels"], pred["scores"])]
        if args.track:
            labels = [f"#{i} {t}" if i else t for i, t in zip(pred["track_ids"].tolist(), labels)]
        out = osp.join(args.output_dir, osp.basename(image_path))
        visualize(out, image_path, pred["bboxes"], labels)
        if args.dump_json:
            extra = {}
            if args.track:
                extra["track_id"] = pred["track_ids"].tolist()
            if args.top_names:                               # per detection: the names of its list, empty slots (label -1) left out
                extra["names"] = [[[texts[c][0], float(s)] for c, s in zip(cs, ss) if c >= 0]
                                  for cs, ss in zip(pred["top_labels"].tolist(), pred["top_scores"].tolist())]
            with open(osp.splitext(out)[0] + ".json", "w") as f:
                json.dump(dict(image=image_path, bboxes=pred["bboxes"].tolist(), scores=pred["scores"].tolist(),
                               labels=pred["labels"].tolist(), texts=[t[0] for t in texts], **extra), f, ensure_ascii=False)
        results.append(pred)
        print(f"[{n + 1}/{len(images)}] {image_path}: {len(pred['scores'])} detections -> {out}", flush=True)
    return results


if __name__ == "__main__":
    main(sys.argv[1:])
