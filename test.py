"""Evaluate a detector checkpoint on the config's test dataset: COCO box mAP (``CocoMetric``) or LVIS mAP
(``LVISMetric``), with the detector and the metric's matching / accumulation on the device.  Command-line compatible
with the reference's ``test.py`` (``config checkpoint --work-dir --out --cfg-options --launcher --local-rank``):

    python test.py config/wedetect_base.py ckpt.pth --text-bank bank.pt
    bash dist_test.sh config/wedetect_base.py ckpt.pth 8 --text-bank bank.pt
    LVIS: --cfg-options test_evaluator.type=LVISMetric test_evaluator.ann_file=... \
          test_dataloader.dataset.dataset.type=YOLOv5LVISV1Dataset test_dataloader.dataset.dataset.ann_file=... ...
          (README.md has the full line; or point test_dataloader / test_evaluator at the LVIS sections of the config)

Flow: contiguous shard of the dataset per rank (``parallel.shard_range``) -> batches of
``test_dataloader.batch_size`` through the test pipeline and ``YOLOWorldDetector.test_step`` -> per-image predictions
on the host, gathered to rank 0 -> rank 0 evaluates, prints the metric lines and writes ``<work_dir>/metrics.json``.
``--out x.pkl`` pickles the per-image result dicts (mmdet ``DumpDetResults``).

Additions: ``--text-bank FILE`` (a precomputed ``[K, 768]`` bank for the K class texts, ``.npy`` / ``.pt``: the XLM-R
tokenizer files are not needed), ``--precision {fp32,fp16x3}``, ``--loader {serial,stream}`` (``stream``: the streamed
loader of wedetect_amd/stream.py — same predictions, decode / upload / steps overlapped) with ``--decode-workers N``, ``--aug-test`` (test-time augmentation: the reference's ``--tta`` block — ``cfg.tta_model`` /
``cfg.tta_pipeline`` or its flip defaults — through wedetect_amd/tta.py; views merged on the device).  ``--show``, ``--show-dir``
and ``--tta`` itself are not implemented and exit with a message.  A batch size above 1 may change predictions in the last bits (split-K choices
of small batches).
"""
import argparse
import json
import os
import os.path as osp
import pickle
import sys
import time

ROOT = osp.dirname(osp.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    from wedetect_amd.cfgfile import DictAction
    parser = argparse.ArgumentParser(description="WeDetect test (and eval) a model")
    parser.add_argument("config", help="test config file path")
    parser.add_argument("checkpoint", help="checkpoint file")
    parser.add_argument("--work-dir", help="the directory to save the file containing evaluation metrics")
    parser.add_argument("--out", type=str, help="dump predictions to a pickle file for offline evaluation")
    parser.add_argument("--show", action="store_true", help="show prediction results (not implemented)")
    parser.add_argument("--show-dir", help="directory where painted images will be saved (not implemented)")
    parser.add_argument("--cfg-options", nargs="+", action=DictAction,
                        help="override some settings in the used config, the key-value pair in xxx=yyy format will be "
                             "merged into config file.")
    parser.add_argument("--launcher", choices=["none", "pytorch", "slurm", "mpi"], default="none", help="job launcher")
    parser.add_argument("--tta", action="store_true", help="test time augmentation (not implemented under this name: see --aug-test)")
    parser.add_argument("--aug-test", action="store_true",
                        help="test-time augmentation: cfg.tta_model / cfg.tta_pipeline, or flip + plain merged with NMS 0.5, 100 per image")
    parser.add_argument("--local_rank", "--local-rank", type=int, default=0)
    parser.add_argument("--text-bank", default=None, help="precomputed [K, 768] class embeddings (.npy / .pt)")
    parser.add_argument("--precision", default=None, choices=["fp32", "fp16x3"])
    parser.add_argument("--loader", default="serial", choices=["serial", "stream"],
                        help="serial: one image at a time through the pipeline (default); stream: decode threads, one batched "
                             "pre-processing launch per batch, pipelined steps (YOLOWorldDetector.predict_stream)")
    parser.add_argument("--decode-workers", type=int, default=None, help="--loader stream: decode threads (default min(12, $OMP_NUM_THREADS or 8))")
    parser.add_argument("--best-class", action="store_true",
                        help="single-label detection: one label per box, the best name of the bank (the reference's multi_label=False)")
    parser.add_argument("--agnostic-nms", action="store_true",
                        help="with --best-class: NMS across labels (mmcv batched_nms class_agnostic=True)")
    parser.add_argument("--sparse-scores", action="store_true",
                        help="multi-label detection without the [B, 8400, K] score tensor: candidates above the threshold as "
                             "per-image lists (same results; a list that overflows falls back to the dense step)")
    parser.add_argument("--sparse-cap", default=65536, type=int, help="with --sparse-scores: list entries per image, rounded up to a power of two and to at least the top-k "
                             "capacity of test_cfg.nms_pre (32768 for 30000); up to 2^20")
    parser.add_argument("--prompt-groups", action="store_true",
                        help="score every class as the best of ALL the prompts its entry of the class-text file lists (synonyms), "
                             "not of the first one; --text-bank then holds (P, 768): one row per prompt, class after class")
    args = parser.parse_args(argv)
    if args.prompt_groups and (args.best_class or args.sparse_scores):
        parser.exit(2, "test.py: --prompt-groups excludes --best-class and --sparse-scores\n")
    if args.prompt_groups and (args.aug_test or args.loader == "stream"):
        parser.exit(2, "test.py: --prompt-groups runs with --loader serial and without --aug-test (the streamed loader and the "
                       "view merge are not built for it)\n")
    if args.sparse_scores and args.best_class:
        parser.exit(2, "test.py: --sparse-scores (multi-label) and --best-class (single-label) exclude each other\n")
    if args.sparse_scores and (args.aug_test or args.loader == "stream"):
        parser.exit(2, "test.py: --sparse-scores runs with --loader serial and without --aug-test (the packed results of the "
                       "streamed loader and the view merge do not carry the sparse status)\n")
    if args.agnostic_nms and not args.best_class:
        parser.exit(2, "test.py: --agnostic-nms needs --best-class\n")
    if args.best_class and args.aug_test:
        parser.exit(2, "test.py: --best-class is not implemented with --aug-test (the view merge ranks (anchor, class) rows)\n")
    if "LOCAL_RANK" not in os.environ:
        os.environ["LOCAL_RANK"] = str(args.local_rank)
    for flag, on in (("--show", args.show), ("--show-dir", args.show_dir)):
        if on:
            parser.exit(2, f"test.py: {flag} is not implemented on this path (visualisation is out of scope); run without it\n")
    if args.tta:
        parser.exit(2, "test.py: --tta is not implemented under this name; test-time augmentation is --aug-test\n")
    if args.aug_test and args.loader == "stream":
        parser.exit(2, "test.py: --aug-test runs with --loader serial only (the streamed loader has no view branches)\n")
    if args.launcher in ("slurm", "mpi"):
        parser.exit(2, f"test.py: --launcher {args.launcher} is not implemented; use --launcher pytorch (dist_test.sh)\n")
    if args.out is not None and not args.out.endswith((".pkl", ".pickle")):
        parser.exit(2, "test.py: the output file must be a pkl file.\n")
    return args


def load_bank(path: str):
    import numpy as np
    import torch
    bank = np.load(path) if path.endswith(".npy") else torch.load(path, map_location="cpu")
    if isinstance(bank, dict):
        bank = bank.get("text_embedding", next(iter(bank.values())))
    return torch.as_tensor(np.asarray(bank), dtype=torch.float32)


def predict_shard(model, dataset, indices, batch_size: int):
    """Per-image result dicts (host tensors) of ``indices``, in order."""
    import torch
    out = []
    idx = list(indices)
    for lo in range(0, len(idx), batch_size):
        infos = [dataset.get_data_info(i) for i in idx[lo:lo + batch_size]]
        items = [dataset.pipeline(info) for info in infos]
        data = dict(inputs=torch.stack([it["inputs"] for it in items]), data_samples=[it["data_samples"] for it in items])
        with torch.no_grad():
            outputs = model.test_step(data)
        for info, o in zip(infos, outputs):
            p = o.pred_instances
            out.append(dict(img_id=int(info["img_id"]), img_path=info.get("img_path"),
                            pred_instances=dict(bboxes=p.bboxes.detach().float().cpu(), scores=p.scores.detach().float().cpu(),
                                                labels=p.labels.detach().long().cpu())))
    return out


def build_tta(cfg):
    """The reference's ``--tta`` block (test.py:94-127): ``cfg.tta_model`` / ``cfg.tta_pipeline`` when the config has them,
    its defaults otherwise (wedetect_amd/tta.py).  -> (tta_model dict without ``module``, tta_pipeline list)."""
    import warnings
    from wedetect_amd import tta
    tta_model, tta_pipeline = cfg.get("tta_model", None), cfg.get("tta_pipeline", None)
    if tta_model is None:
        warnings.warn("Cannot find ``tta_model`` in config, we will set it as default.")
        tta_model = dict(tta.DEFAULT_TTA_MODEL)
    if tta_pipeline is None:
        warnings.warn("Cannot find ``tta_pipeline`` in config, we will set it as default.")
        data_cfg = cfg.test_dataloader.dataset                # the reference descends to the innermost dataset; the shipped
        test_pipeline = data_cfg.get("pipeline", None)        # configs keep the pipeline on the MultiModalDataset wrapper
        while "dataset" in data_cfg:
            data_cfg = data_cfg["dataset"]
            test_pipeline = data_cfg.get("pipeline", test_pipeline)
        if test_pipeline is None:
            raise SystemExit("--aug-test: the test dataset has no pipeline to derive the TTA pipeline from")
        tta_pipeline = tta.default_tta_pipeline(test_pipeline)
    return dict(tta_model), list(tta_pipeline)


def predict_shard_tta(tta_model, dataset, pipeline, indices, batch_size: int):
    """``predict_shard`` under test-time augmentation: ``pipeline`` ends in a ``TestTimeAug`` (every image comes out as a list
    of views); a batch is collated per view (``tta.collate_views``) and goes through ``DetTTAModel.test_step``."""
    from wedetect_amd.tta import collate_views
    out = []
    idx = list(indices)
    for lo in range(0, len(idx), batch_size):
        infos = [dataset.get_data_info(i) for i in idx[lo:lo + batch_size]]
        outputs = tta_model.test_step(collate_views([pipeline(dict(info)) for info in infos]))
        for info, o in zip(infos, outputs):
            p = o.pred_instances
            out.append(dict(img_id=int(info["img_id"]), img_path=info.get("img_path"),
                            pred_instances=dict(bboxes=p.bboxes.float(), scores=p.scores.float(), labels=p.labels.long())))
    return out


def predict_shard_stream(model, dataset, indices, batch_size: int, decode_workers=None, stats=None):
    """``predict_shard`` through the streamed loader: the same result dicts, in the same order."""
    infos = [dataset.get_data_info(i) for i in indices]
    out = []
    for info, o in zip(infos, model.predict_stream(infos, batch_size, dataset.pipeline, decode_workers=decode_workers, stats=stats)):
        p = o.pred_instances
        out.append(dict(img_id=int(info["img_id"]), img_path=info.get("img_path"),
                        pred_instances=dict(bboxes=p.bboxes.float(), scores=p.scores.float(), labels=p.labels.long())))
    return out


def main(argv=None):
    args = parse_args(argv)
    import torch
    import torch.distributed as dist
    from wedetect_amd import parallel
    from wedetect_amd.apis import init_detector
    from wedetect_amd.cfgfile import Config
    from wedetect_amd.datasets import build_dataset, build_metric, metric_lines

    cfg = Config.fromfile(args.config)
    if args.cfg_options is not None:
        cfg.merge_from_dict(args.cfg_options)
    if args.best_class:
        cfg.merge_from_dict({"model.best_class": True, "model.agnostic_nms": bool(args.agnostic_nms)})
    if args.sparse_scores:
        cfg.merge_from_dict({"model.sparse_scores": True, "model.sparse_cap": int(args.sparse_cap)})
    if args.prompt_groups:
        cfg.merge_from_dict({"model.prompt_groups": True})
    if args.work_dir is not None:
        cfg.work_dir = args.work_dir
    elif cfg.get("work_dir", None) is None:
        cfg.work_dir = osp.join("./work_dirs", osp.splitext(osp.basename(args.config))[0])

    if args.launcher == "pytorch":
        dist.init_process_group("gloo")                 # the gather moves host objects only
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    local = int(os.environ.get("LOCAL_RANK", args.local_rank))
    device = f"cuda:{local}"
    torch.cuda.set_device(local)

    dataset = build_dataset(cfg.test_dataloader.dataset)
    texts = dataset.class_texts
    if texts is None:
        texts = [[name] for name in dataset.metainfo["classes"]]
        dataset.class_texts = texts
    model = init_detector(cfg, checkpoint=args.checkpoint, device=device, precision=args.precision)
    if args.text_bank:
        bank = load_bank(args.text_bank)
        if args.prompt_groups:
            n_prompts = sum(len(t) for t in texts)
            if tuple(bank.shape) != (n_prompts, 768):
                raise SystemExit(f"--text-bank holds {tuple(bank.shape)}, expected ({n_prompts}, 768) with --prompt-groups: one row "
                                 f"per prompt of the {len(texts)} classes, class after class")
        elif tuple(bank.shape) != (len(texts), 768):
            raise SystemExit(f"--text-bank holds {tuple(bank.shape)}, expected ({len(texts)}, 768): one row per class text")
        model.set_text_embeddings(bank.to(device), texts)
    elif args.prompt_groups:
        model.reparameterize(texts)                           # every prompt of every class: the samples' first captions find this bank
    batch_size = int(cfg.test_dataloader.get("batch_size", 1))
    shard = parallel.shard_range(len(dataset), world, rank)
    t0 = time.time()
    if args.aug_test:
        from wedetect_amd.pipeline import Compose
        from wedetect_amd.registry import MODELS
        tta_model, tta_pipeline = build_tta(cfg)
        preds = predict_shard_tta(MODELS.build(dict(tta_model, module=model)), dataset, Compose(tta_pipeline), shard, batch_size)
    elif args.loader == "stream":
        preds = predict_shard_stream(model, dataset, shard, batch_size, args.decode_workers)
    else:
        preds = predict_shard(model, dataset, shard, batch_size)
    print(f"[rank {rank}] {len(preds)} images in {time.time() - t0:.1f} s", flush=True)
    preds = parallel.gather_to_rank0(preds)
    if rank == 0:
        if args.out:
            d = osp.dirname(osp.abspath(args.out))
            os.makedirs(d, exist_ok=True)
            with open(args.out, "wb") as f:
                pickle.dump(preds, f)
        metric = build_metric(cfg.test_evaluator)
        metric.process([dict(img_id=p["img_id"], bboxes=p["pred_instances"]["bboxes"].numpy(),
                             scores=p["pred_instances"]["scores"].numpy(),
                             labels=p["pred_instances"]["labels"].numpy()) for p in preds])
        metrics = metric.compute_metrics(device=device)
        if metrics:
            for line in metric_lines(metric.eval, metric.lvis):
                print(line)
            for name, ap in metric.eval.get("classwise", []):
                print(f"{name:<24} {ap:.3f}")
            print(json.dumps(metrics))
            os.makedirs(cfg.work_dir, exist_ok=True)
            with open(osp.join(cfg.work_dir, "metrics.json"), "w") as f:
                json.dump(metrics, f, indent=1)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    return metrics if rank == 0 else None


if __name__ == "__main__":
    main(sys.argv[1:])
