#!/usr/bin/env python3
"""`label`, `decode`, `postprocess`, `postprocess_fg`, `evaluate_prediction`, `evaluate`, `visualize` and `validate` tasks with the reference driver's interface
(reference: experiments/run_ppp.py -- argument names :157-267, task dispatch :1974-2293,
``decode`` :682-746, ``vote_instances`` / ``vote_instances_sample`` :1054-1190, ``postprocess``
:2230-2259).  The reference's ``postprocess`` has two branches: ``process_instances`` is this driver's
``--do postprocess``; ``process_fg_prediction`` (:2234-2245) is a task of its own here,
``--do postprocess_fg``, and stays refused under ``--do postprocess``.

``evaluate_prediction`` (:1300-1443, the reference's ``[evaluation] prediction_only_test`` branch
:2207-2211) scores the dense prediction against ``[data] test_data`` before any instance is voted.

``evaluate`` (:1193-1262, :1447-1536): the voted instance maps of --output-folder scored against the ground
truth instances (`evaluate_instances`: this project's own definitions, the reference's evaluation package
is not vendored).

``visualize`` (:1539-1606): patch mosaics of the prediction (``show_patches``) and instance pictures
(``show_instances``).

``validate`` (:779-1051): every parameter set of ``[validation]`` voted and scored on the predictions of
--pred-folder, ``results.json`` and the best set (`validate.validate_checkpoints`; ``--val-id N`` runs set N only).
A sample is loaded once for all its sets.

Only the tasks on this repository's path are provided; training and prediction stay with the reference.  Usage, as in the reference README:

    python -m patchperpix_amd.run_ppp --setup setup01 --config default.toml --do label \
        --pred-folder <dir with *.zarr|*.hdf|*.npy> --output-folder <dir> [--sample NAME]

Config: the reference's TOML files are read unchanged ([vote_instances], [model], [prediction],
[visualize], [general], [data], [evaluation], [postprocessing]).
"""
import argparse
import glob
import logging
import os
import sys
import time

logger = logging.getLogger(__name__)


def load_config(paths):
    try:
        import tomllib as toml_reader   # Python >= 3.11
    except ImportError:
        import tomli as toml_reader
    config = {}
    from .vote_instances.vote_instances import merge_dicts
    for p in paths:
        with open(p, "rb") as f:
            config = merge_dicts(config, toml_reader.load(f))
    return config


def get_list_samples(pred_folder, fmt, only=None):
    names = sorted(os.path.splitext(os.path.basename(p))[0]
                   for p in glob.glob(os.path.join(pred_folder, "*." + fmt)))
    return [n for n in names if only is None or only in n]


def stitch_kwargs(config):
    """what `vote_instances_sample` hands ``stitch_patch_graph.main`` for a ``blockwise`` sample (run_ppp.py:1160-1170)"""
    cfg, pred = config["vote_instances"], config["prediction"]
    extra = {}
    if cfg.get("vote_from_code", False):
        # project-own option: a sample that holds the code is decoded into rows
        # for its foreground voxels and voted from them; what the `decode` task is given
        extra = dict(code_key=pred.get("code_key"), checkpoint_file=config.get("_checkpoint"))
        if "autoencoder" not in config["model"] and config.get("autoencoder"):
            extra["included_ae_config"] = config["autoencoder"]
        for k in ("use_swa", "decode_batch_size"):
            if k in pred and k not in cfg and k not in config["model"]:
                extra[k] = pred[k]
    # (written as one call's keyword arguments so that a name given twice is refused, as it always was)
    return (lambda **kw: kw)(
        **cfg, **config["model"], **config.get("visualize", {}), **extra,
        aff_key=pred.get("aff_key"), numinst_key=pred.get("numinst_key"),
        fg_key=pred.get("fg_key"), fg_folder=pred.get("fg_folder"),
        fg_thresh=pred.get("fg_thresh"))


def vote_instances_sample(config, pred_folder, output_folder, sample):
    """run_ppp.py:1119-1190."""
    from . import vote_instances as vi
    cfg = config["vote_instances"]
    cfg["result_folder"] = output_folder
    cfg["check_required"] = False
    out_fmt = cfg.get("output_format", "hdf")
    output_fn = os.path.join(output_folder, os.path.basename(sample) + "." + out_fmt)
    if not config.get("general", {}).get("overwrite", False) and os.path.exists(output_fn):
        logger.info("Skipping vote instances for %s. Already exists!", output_fn)
        return
    pred_fmt = config["prediction"]["output_format"]
    pred_file = os.path.join(pred_folder, sample + "." + pred_fmt)
    pred = config["prediction"]
    if cfg.get("vote_from_code", False) and not cfg.get("blockwise", False):
        raise NotImplementedError("[vote_instances] vote_from_code = true needs blockwise = true")
    if cfg.get("blockwise", False):
        vi.stitch_patch_graph.main(pred_file, **stitch_kwargs(config))
    else:
        cfg["affinities"] = pred_file
        vi.vote_instances.main(**cfg, **config["model"], numinst_key=pred.get("numinst_key"),
                               aff_key=pred.get("aff_key"), fg_key=pred.get("fg_key"))


def label_batched(config, pred_folder, output_folder, samples):
    """`label` with ``[vote_instances] batch_2d = N``: 2-d samples of equal shape are voted N at a
    time in one call (vote_instances.do_all_batched); the result files are those of a run
    without it."""
    from . import vote_instances as vi
    cfg = dict(config["vote_instances"], result_folder=output_folder, check_required=False)
    out_fmt = cfg.get("output_format", "hdf")
    pred_fmt = config["prediction"]["output_format"]
    todo = []
    for sample in samples:
        output_fn = os.path.join(output_folder, os.path.basename(sample) + "." + out_fmt)
        if not config.get("general", {}).get("overwrite", False) and os.path.exists(output_fn):
            logger.info("Skipping vote instances for %s. Already exists!", output_fn)
            continue
        todo.append(os.path.join(pred_folder, sample + "." + pred_fmt))
    if not todo:
        return
    pred = config["prediction"]
    cfg.pop("affinities", None)
    vi.vote_instances.main(**cfg, **config["model"], aff_files=todo, numinst_key=pred.get("numinst_key"),
                           aff_key=pred.get("aff_key"), fg_key=pred.get("fg_key"))


def label(args, config):
    samples = get_list_samples(args.pred_folder, config["prediction"]["output_format"],
                               args.sample)
    os.makedirs(args.output_folder, exist_ok=True)
    cfg = config["vote_instances"]
    if cfg.get("vote_from_code", False) and not cfg.get("blockwise", False):
        raise NotImplementedError("[vote_instances] vote_from_code = true needs blockwise = true")
    config["_checkpoint"] = args.checkpoint
    if int(cfg.get("batch_2d") or 0) > 1 and not cfg.get("blockwise", False):
        t0 = time.time()
        label_batched(config, args.pred_folder, args.output_folder, samples)
        logger.info("time vote_instances (batch_2d = %d, %d samples): %.2fs", int(cfg["batch_2d"]),
                    len(samples), time.time() - t0)
        return
    for idx, sample in enumerate(samples):
        t0 = time.time()
        print("labelling {}/{}: {}".format(idx, len(samples), sample))
        vote_instances_sample(config, args.pred_folder, args.output_folder, sample)
        logger.info("time vote_instances_sample: %.2fs", time.time() - t0)


def decode(args, config):
    from . import decode as dec
    fmt = config["prediction"]["output_format"]
    samples = [os.path.join(args.pred_folder, s + "." + fmt)
               for s in get_list_samples(args.pred_folder, fmt, args.sample)]
    os.makedirs(args.output_folder, exist_ok=True)
    dec.decode(checkpoint_file=args.checkpoint, output_folder=args.output_folder, samples=samples,
               included_ae_config=config.get("autoencoder") or config["model"].get("autoencoder"),
               **config["model"], **config["prediction"], **config.get("data", {}))


def postprocess(args, config):
    """run_ppp.py:2230-2259: the result files ``*.<vote_instances.output_format>`` of --output-folder,
    ``res_key`` from [evaluation], everything else from [postprocessing]."""
    from . import postprocess as post
    cfg = config.get("postprocessing", {})
    if cfg.get("process_fg_prediction", False):
        raise NotImplementedError("[postprocessing] process_fg_prediction = true is not served by --do postprocess: "
                                  "run that branch as --do postprocess_fg; unset it to run process_instances")
    if cfg.get("process_instances", False):
        fmt = config["vote_instances"].get("output_format", "hdf")
        samples = [os.path.join(args.output_folder, s + "." + fmt)
                   for s in get_list_samples(args.output_folder, fmt, args.sample)]
        t0 = time.time()
        post.postprocess_instances(samples, args.output_folder, res_key=config["evaluation"]["res_key"], **cfg)
        logger.info("time postprocess_instances (%d samples): %.2fs", len(samples), time.time() - t0)


def postprocess_fg(args, config):
    """run_ppp.py:2234-2245, the ``process_fg_prediction`` branch as a task of its own: the prediction
    files ``*.<prediction.output_format>`` of --pred-folder, ``fg_key`` from [prediction], everything else
    from [postprocessing]; one ``<sample>.hdf`` per file in --output-folder."""
    from . import postprocess as post
    fmt = config["prediction"]["output_format"]
    samples = [os.path.join(args.pred_folder, s + "." + fmt)
               for s in get_list_samples(args.pred_folder, fmt, args.sample)]
    os.makedirs(args.output_folder, exist_ok=True)
    t0 = time.time()
    post.postprocess_fg(samples, args.output_folder, fg_key=config["prediction"]["fg_key"],
                        **config.get("postprocessing", {}))
    logger.info("time postprocess_fg (%d samples): %.2fs", len(samples), time.time() - t0)


def evaluate_prediction(args, config):
    """run_ppp.py:1370-1443: every ``*.<prediction.output_format>`` of --pred-folder against the ground truth
    of ``[data] test_data`` -- a ``.zarr`` / ``.hdf`` file with ``<sample>/<gt_key>``, or a folder of
    ``<sample>.<input_format>`` files with ``gt_key`` -- by ``[evaluation.prediction]``'s switches
    (``eval_numinst_prediction``, ``eval_fg_prediction``, ``eval_patch_prediction``).  The per-sample dicts
    go to ``prediction_metrics.json`` in --output-folder (this project's file, in place of the reference's
    ``summarize_metric_dict``); returns (metrics, ths) as the reference does."""
    import json
    from . import evaluate_prediction as ev
    fmt = config["prediction"]["output_format"]
    data = config["data"]["test_data"]
    samples = get_list_samples(args.pred_folder, fmt, args.sample)
    os.makedirs(args.output_folder, exist_ok=True)
    t0 = time.time()
    metric_dicts = [ev.evaluate_prediction_sample(config, s, data, args.pred_folder, fmt, args.output_folder)
                    for s in samples]
    with open(os.path.join(args.output_folder, "prediction_metrics.json"), "w") as f:
        json.dump({s: ev.jsonable(m) for s, m in zip(samples, metric_dicts)}, f, indent=1, sort_keys=True)
    result = ev.summarize(metric_dicts, samples, config["evaluation"]["metric"])
    logger.info("time evaluate_prediction (%d samples): %.2fs", len(samples), time.time() - t0)
    return result


def evaluate(args, config):
    """run_ppp.py:1447-1536 with `evaluate_sample` (:1193-1262), without the ``conic``, ``add_partly_val`` and
    ``Parallel`` branches; ``[evaluation] evaluate_skeleton_coverage``, ``[evaluation] print_f_factor_perc_gt_0_8`` and
    ``[data] add_partly_val`` are refused by name.  With ``one_instance_per_channel``, ``[data]
    one_instance_per_channel_gt`` names the ground-truth dataset in place of ``gt_key`` (:1215-1218), for every layout
    of ``test_data`` as in the reference.  The samples are the
    ``*.<vote_instances.output_format>`` files of --output-folder; the ground truth comes from ``[data]
    test_data`` as `evaluate_prediction` resolves it: a ``.zarr`` / ``.hdf`` file with ``<sample>/<gt_key>``, or a
    folder of ``<sample>.<input_format>`` files with ``gt_key``.  ``res_key`` and the switches come from
    ``[evaluation]``, ``overlapping_inst`` from ``[vote_instances] one_instance_per_channel``.  Per sample
    `evaluate_instances.evaluate_file` writes ``<output_folder>/<sample>.toml`` and ``<metric> sample <name>:
    <value>`` is logged.  With ``[evaluation] summary`` (a list of dotted keys) ``summary.csv`` goes to
    --output-folder: the header ``sample`` plus the keys, one row per sample, floats by repr -- this project's
    own format, as ``prediction_metrics.json`` is.  Returns the mean of ``[evaluation] metric`` over the
    samples."""
    return evaluate_folder(config, config["data"]["test_data"], args.output_folder, args.output_folder, args.sample)


def evaluate_folder(config, data, inst_folder, eval_folder, sample=None):
    """The body of `evaluate` (run_ppp.py:1447-1536 takes the same five): the ``*.<vote_instances.output_format>``
    files of ``inst_folder`` (those whose name contains ``sample``) against the ground truth ``data``; the
    per-sample ``.toml`` files and ``summary.csv`` go to ``eval_folder``.  `evaluate` calls it with ``[data]
    test_data`` and --output-folder for both folders, `validate` with ``[data] val_data`` and one folder pair
    per parameter set."""
    import numpy as np
    from . import evaluate_instances as ei
    cfg = config["evaluation"]
    if cfg.get("evaluate_skeleton_coverage"):
        raise NotImplementedError("[evaluation] evaluate_skeleton_coverage is not provided by this repository; unset it")
    if cfg.get("print_f_factor_perc_gt_0_8"):
        raise NotImplementedError("[evaluation] print_f_factor_perc_gt_0_8 is not provided by this repository; unset it")
    if config["data"].get("add_partly_val"):
        raise NotImplementedError("[data] add_partly_val is not provided by this repository; unset it")
    fmt = config["vote_instances"].get("output_format", "hdf")
    samples = get_list_samples(inst_folder, fmt, sample)
    t0 = time.time()
    metrics, dicts = {}, []
    for sample in samples:
        if data.rstrip("/").endswith(("zarr", "hdf")):
            gt_path, gt_key = data, sample + "/" + config["data"]["gt_key"]
        else:
            gt_path = os.path.join(data, sample + "." + config["data"]["input_format"])
            gt_key = config["data"]["gt_key"]
        if config["vote_instances"].get("one_instance_per_channel") and config["data"].get("one_instance_per_channel_gt"):
            gt_key = config["data"]["one_instance_per_channel_gt"]
            logger.info("call evaluation with key %s", gt_key)
        metric_dict = ei.evaluate_file(
            os.path.join(inst_folder, sample + "." + fmt), gt_path, res_key=cfg["res_key"], gt_key=gt_key,
            out_dir=eval_folder, suffix="",
            foreground_only=cfg.get("foreground_only", False),
            debug=config.get("general", {}).get("debug", False),
            from_scratch=cfg.get("from_scratch", False),
            overlapping_inst=config["vote_instances"].get("one_instance_per_channel", False),
            use_linear_sum_assignment=cfg.get("use_linear_sum_assignment", False),
            metric=cfg.get("metric", None), filterSz=cfg.get("filterSz", None),
            localization_criterion=cfg.get("localization_criterion", "iou"),
            remove_small_components=cfg.get("remove_small_components", None),
            keep_gt_shape=cfg.get("keep_gt_shape", False), partly=False,
            visualize=cfg.get("visualize", False), visualize_type=cfg.get("visualize_type", "nuclei"),
            assignment_strategy=cfg.get("assignment_strategy", "hungarian"),
            evaluate_false_labels=cfg.get("evaluate_false_labels", False),
            unique_false_labels=cfg.get("unique_false_labels", False),
            add_general_metrics=cfg.get("add_general_metrics", []),
            add_multi_thresh_metrics=cfg.get("add_multi_thresh_metrics", []))
        dicts.append(metric_dict)
        value = float(ei.lookup(metric_dict, cfg["metric"]))
        logger.info("%s sample %-19s: %.4f", cfg["metric"], sample, value)
        metrics[sample] = value
    if "summary" in cfg:
        with open(os.path.join(eval_folder, "summary.csv"), "w") as f:
            f.write(",".join(["sample"] + list(cfg["summary"])) + "\n")
            for sample, metric_dict in zip(samples, dicts):
                cells = [ei.lookup(metric_dict, k) for k in cfg["summary"]]
                f.write(",".join([sample] + [repr(c) if isinstance(c, float) else str(c) for c in cells]) + "\n")
    logger.info("time evaluate (%d samples): %.2fs", len(samples), time.time() - t0)
    return float(np.mean(list(metrics.values()))) if metrics else float("nan")


def visualize(args, config):
    """run_ppp.py:1539-1606, by ``[visualize]``'s switches, for the samples of ``samples_to_visualize``.

    ``show_patches``: for every such sample present in --pred-folder as ``<sample>.<prediction.output_format>``
    the patch mosaic of ``aff_key`` goes to ``<pred_folder>/<sample>.hdf``, dataset ``<aff_key>_patched``
    (`visualize.visualize_patches`); a sample whose ``.hdf`` exists is skipped.

    ``show_instances``: ``vote_instances`` of ``<output_folder>/<sample>.<vote_instances.output_format>`` as
    ``<output_folder>/<sample>.png`` (`visualize.visualize_instances`), with ``max_axis = 0`` when
    ``one_instance_per_channel`` is set; a sample whose PNG exists is skipped.  The reference loops over the
    validation's parameter sets here and looks into one result folder per set, but its loop cannot run as
    written: it reads ``params``, a name that exists only in the reference's ``main`` (:1572).  This task
    serves the ONE folder the `label` task writes, --output-folder."""
    from .visualize import visualize_instances, visualize_patches
    cfg = config.get("visualize", {})
    wanted = cfg.get("samples_to_visualize", [])
    if cfg.get("show_patches"):
        fmt = config["prediction"]["output_format"]
        samples = get_list_samples(args.pred_folder, fmt)
        aff_key = config["prediction"].get("aff_key", "volumes/pred_affs")
        for sample in wanted:
            if sample not in samples:
                continue
            infn = os.path.join(args.pred_folder, sample + "." + fmt)
            outfn = os.path.join(args.pred_folder, sample + ".hdf")
            if os.path.exists(outfn):
                logger.info("Skipping patch mosaic for %s. Already exists!", outfn)
                continue
            t0 = time.time()
            visualize_patches(infn, config["model"]["patchshape"], in_key=aff_key, out_file=outfn,
                              out_key=aff_key + "_patched")
            logger.info("time visualize_patches %s: %.2fs", sample, time.time() - t0)
    if cfg.get("show_instances"):
        fmt = config["vote_instances"].get("output_format", "hdf")
        samples = get_list_samples(args.output_folder, fmt)
        max_axis = 0 if config["vote_instances"].get("one_instance_per_channel") else None
        for sample in wanted:
            if sample not in samples:
                continue
            outfn = os.path.join(args.output_folder, sample + ".png")
            if os.path.exists(outfn):
                logger.info("Skipping instance picture %s. Already exists!", outfn)
                continue
            visualize_instances(os.path.join(args.output_folder, sample + "." + fmt), "vote_instances", outfn,
                                max_axis=max_axis)


def validate(args, config):
    """run_ppp.py:919-1051 on predictions that exist: `validate.validate_checkpoints`."""
    from . import validate as val
    config["_checkpoint"] = args.checkpoint
    return val.validate_checkpoints(config, args.pred_folder, args.output_folder, sample=args.sample,
                                    val_id=args.val_id)


def main(argv=None):
    from patchperpix_amd import backend as _backend
    _backend.tune_host_allocator(cli=True)     # (main(argv) IS the program, also behind a console script)
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config", action="append", required=True)
    ap.add_argument("-a", "--app", default="flylight")
    ap.add_argument("-s", "--setup", default="setup01")
    ap.add_argument("-d", "--do", nargs="+", default=["label"], choices=["label", "decode", "postprocess", "postprocess_fg", "evaluate_prediction", "evaluate", "visualize", "validate"])
    ap.add_argument("--pred-folder", required=True)
    ap.add_argument("--output-folder", required=True)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--sample", default=None)
    ap.add_argument("--val-id", type=int, default=-1, help="validate: run only this parameter set (run_ppp.py:956)")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    config = load_config(args.config)
    for task in args.do:
        {"label": label, "decode": decode, "postprocess": postprocess, "postprocess_fg": postprocess_fg,
         "evaluate_prediction": evaluate_prediction, "evaluate": evaluate, "visualize": visualize, "validate": validate}[task](args, config)


if __name__ == "__main__":
    main(sys.argv[1:])
