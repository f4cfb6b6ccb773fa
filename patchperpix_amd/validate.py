"""The `validate` task: vote and score every parameter set of ``[validation]`` and return the best one
(reference: experiments/run_ppp.py -- ``validate_checkpoint`` :779-853, ``get_postprocessing_params`` :856-872,
``named_product`` / ``named_zip`` / ``named_params`` :875-916, ``validate_checkpoints`` :919-1051,
``select_validation_data`` :760-775).

The reference loops set-major: for every set it opens, decompresses and uploads every sample again.  The
results do not depend on the order, so the sweep here is sample-major: inside a checkpoint a sample is opened
ONCE (`SampleSession`), its affinities are read, tested for logits and mapped once and -- when they fit -- kept
on the device, and every set is voted from that copy.  What depends on a set (the numinst and
foreground fields, the bounding box, the cover mask) is made again for every set.
"""
import contextlib
import copy
import itertools
import json
import logging
import os
import time

import numpy as np

logger = logging.getLogger(__name__)


# ------------------------------------------------------------------------------------------------
# the parameter sets
# ------------------------------------------------------------------------------------------------
def get_postprocessing_params(config, params_product_list, params_zip_list, test_config):
    """run_ppp.py:856-872: (params_zip, params_product), name -> list of values from ``config`` (the
    ``[validation]`` section); an empty list (or no section) falls back to ``[test_config[name]]``."""
    def values(names):
        return {p: [test_config[p]] if config is None or config[p] == [] else config[p] for p in names}
    params_product = values(params_product_list)
    return values(params_zip_list), params_product


def named_product(**items):
    """run_ppp.py:875-882"""
    if items:
        for res in itertools.product(*items.values()):
            yield dict(zip(items.keys(), res))
    else:
        yield {}


def named_zip(**items):
    """run_ppp.py:884-891"""
    if items:
        for res in zip(*items.values()):
            yield dict(zip(items.keys(), res))
    else:
        yield {}


def named_params(params_zip, params_product):
    """run_ppp.py:894-916: the zip is the outer loop, the product the inner one; a set is the zip dict with the
    product dict merged over it.  With neither, one empty set."""
    from .vote_instances.vote_instances import merge_dicts
    if params_zip and params_product:
        for z in named_zip(**params_zip):
            for p in named_product(**params_product):
                yield merge_dicts(copy.deepcopy(z), p)
    elif params_zip:
        yield from named_zip(**params_zip)
    elif params_product:
        yield from named_product(**params_product)
    else:
        yield {}


def params_str(params):
    """run_ppp.py:784-787: one folder component per parameter"""
    out = []
    for k, v in params.items():
        s = str(v).replace(".", "_").replace(" ", "")
        for ch in ",[]()":
            s = s.replace(ch, "_")
        out.append(k + "_" + s)
    return out


def param_sets_of(config):
    """run_ppp.py:942-950: the sets of ``[validation]`` (``params_product``, older files: ``params``, and
    ``params_zip``) over ``[vote_instances]``"""
    val = config["validation"]
    return list(named_params(*get_postprocessing_params(
        val, val.get("params_product", val.get("params", [])), val.get("params_zip", []),
        config["vote_instances"])))


# ------------------------------------------------------------------------------------------------
# one load per sample
# ------------------------------------------------------------------------------------------------
class CachingReader:
    """A container (zarr group / HDF5 file) that hands every dataset out as ONE host array, read on first use;
    ``reads[key]`` counts the reads that reached the container.  `PredictionFile` views on it share the arrays:
    they copy what they hand on (``np.array``), the cached arrays are never written to.

    Two exceptions keep a large array from staying on the host: a key in ``raw`` is handed out as the container's
    own dataset and never cached (a streamed prediction), and `keep_channel` cuts a cached array back to the one
    channel that `PredictionFile.foreground` may still ask for."""

    def __init__(self, container):
        self.f, self.cache, self.reads, self.raw = container, {}, {}, set()

    def keys(self):
        return self.f.keys()

    def __contains__(self, key):
        return key in self.f

    def read(self, key):
        arr = np.array(self.f[key])
        arr.setflags(write=False)
        self.reads[key] = self.reads.get(key, 0) + 1
        return arr

    def __getitem__(self, key):
        if key in self.raw:
            self.cache.pop(key, None)
            return self.f[key]
        if key not in self.cache:
            self.cache[key] = self.read(key)
        return self.cache[key]

    def keep_channel(self, key, index):
        """forget the cached array of ``key`` but for ``[index]``: what stands in for it has the array's shape,
        serves that channel from memory and reads the container again (counted) for anything else"""
        arr = self.cache.get(key)
        if isinstance(arr, np.ndarray) and 0 <= index < arr.shape[0]:
            self.cache[key] = _OneChannel(self, key, arr, index)


class _OneChannel:
    def __init__(self, reader, key, arr, index):
        self.reader, self.key, self.index = reader, key, int(index)
        self.shape, self.dtype = arr.shape, arr.dtype
        self.kept = arr[index].copy()
        self.kept.setflags(write=False)

    def __getitem__(self, sel):
        if isinstance(sel, (int, np.integer)) and int(sel) == self.index:
            return self.kept
        return self.reader.read(self.key)[sel]

    def __array__(self, dtype=None, copy=None):
        arr = self.reader.read(self.key)
        return arr if dtype is None else arr.astype(dtype)


def resident_mode():
    mode = os.environ.get("PPP_VALIDATE_RESIDENT", "auto")
    if mode not in ("auto", "device", "host", "off"):
        raise ValueError("PPP_VALIDATE_RESIDENT=%s: one of auto, device, host, off" % mode)
    return mode


class SampleSession:
    """One prediction file, open for all the parameter sets of a sweep.  `vote` runs one set and writes its
    result file, the same bytes `run_ppp.vote_instances_sample` writes for that configuration.

    Kept per sample:

    * every dataset the loaders ask for, read once (`CachingReader`); the numinst and foreground FIELDS are
      computed per set by `PredictionFile` on that reader, with the set's kwargs;
    * the affinities: read, decompressed, tested for logits and mapped through ``expit`` once, exactly as
      ``loadAffinities`` does it.  When their bytes are at most a quarter of the free HBM at that moment they are
      uploaded once and stay on the device in their stored type -- the bounding-box crop of a set is then a
      device copy (``h2d_copies`` stays at 1).  Above that size the host array is kept and the crop is uploaded
      per set.  ``PPP_VALIDATE_RESIDENT=device|host`` forces either.  The reader's own copy of the stored array is
      then cut back to the centre channel, the one part the foreground may still be read from;
    * with ``vote_from_code`` the rows (`CompactPrediction`), decoded once;
    * for a prediction that `tiling._want_stream` streams: one ``ZarrProvider``, and the logits test, once.  The
      array itself is never cached: the tiles are read per set, and a foreground taken from the centre channel
      reads that channel from the open dataset, as `tiling._stitch_load` does.

    ``h2d_copies`` is the number of host -> device copies of a prediction that `backend.to_device_pred` made while
    this session voted (``backend.PRED_UPLOADS``), ``times`` the seconds spent in the load (without the upload),
    the one-time upload, and the vote.

    NOT resident: ``blockwise = false`` samples (``batch_2d`` included), ``blockwise_semantics = "reference"``,
    ``.npy`` predictions and ``PPP_VALIDATE_RESIDENT=off`` go through `run_ppp.vote_instances_sample` per set,
    unchanged: correct, but every set loads the sample again.

    Nothing of one set reaches the next: `tiling._stitch_vote` works on copies of the cover mask and the
    fields, and the ``[vote_instances]`` dict that `vote_instances_sample` writes to is a deep copy per set."""

    def __init__(self, pred_folder, sample, pred_fmt):
        from .vote_instances import io_hdflike
        self.pred_folder, self.sample = pred_folder, sample
        self.pred_file = os.path.join(pred_folder, sample + "." + pred_fmt)
        self.mode = resident_mode()
        self.stack = contextlib.ExitStack()
        self.reader = None
        if self.mode != "off" and self.pred_file.rstrip("/").endswith((".zarr", ".hdf")):
            self.reader = CachingReader(self.stack.enter_context(io_hdflike.open_container(self.pred_file, "r")))
        self._aff = {}          # load key -> host array or device tensor
        self._compact = {}      # decode key -> CompactPrediction
        self._provider = {}     # aff_key -> ZarrProvider
        self.h2d_copies = 0     # host -> device copies of the affinities, as backend.to_device_pred counted them
        self.sets_voted = 0
        self.times = {"load": 0.0, "upload": 0.0, "vote": 0.0}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        self._aff.clear()
        self._compact.clear()
        self._provider.clear()
        if self.reader is not None:
            self.reader.cache.clear()
        self.stack.close()

    @property
    def reads(self):
        return {} if self.reader is None else self.reader.reads

    # ---- one set ---------------------------------------------------------------------------------
    def vote(self, config, inst_folder):
        from . import backend
        uploads = backend.PRED_UPLOADS
        try:
            self._vote(copy.deepcopy(config), inst_folder)
        finally:
            self.h2d_copies += backend.PRED_UPLOADS - uploads

    def _vote(self, config, inst_folder):
        from . import run_ppp, tiling
        cfg = config["vote_instances"]
        self.sets_voted += 1
        if self.reader is None or not cfg.get("blockwise", False) or \
                cfg.get("blockwise_semantics", "whole_volume") == "reference":
            t0 = time.perf_counter()
            run_ppp.vote_instances_sample(config, self.pred_folder, inst_folder, self.sample)
            self.times["vote"] += time.perf_counter() - t0
            return
        cfg["result_folder"] = inst_folder
        cfg["check_required"] = False
        kw = run_ppp.stitch_kwargs(config)
        kw.pop("blockwise_semantics", None)
        kw.pop("result_folder")
        patchshape = np.array(kw.pop("patchshape"))
        t0, upload = time.perf_counter(), self.times["upload"]
        loaded = self._load(patchshape, kw)
        t1 = time.perf_counter()
        self.times["load"] += (t1 - t0) - (self.times["upload"] - upload)
        if loaded is None:
            return
        tiling._stitch_vote(loaded[0], loaded[1], loaded[2], self.pred_file, inst_folder, patchshape, kw)
        self.times["vote"] += time.perf_counter() - t1

    # ---- tiling._stitch_load on the open container -------------------------------------------------
    def _load(self, patchshape, kw):
        from . import tiling
        from .vote_instances import utilVoteInstances as util
        f = self.reader
        from_code = bool(kw.pop("vote_from_code", False))
        kw.pop("load_on_device", None)      # (the session keeps its host load: its sample stays resident anyway)
        if from_code and (kw.get("code_key") or "volumes/pred_code") in f:
            key = repr([kw.get(k) for k in ("code_key", "numinst_key", "fg_key", "fg_thresh", "decode_batch_size",
                                            "checkpoint_file", "logits", "use_swa")] + [patchshape.tolist()])
            if key not in self._compact:
                self._compact[key] = tiling._compact_from_code(None, self.pred_file, patchshape, kw)[0]
            numinst = util.maybeLoadNuminst(f, **kw)
            foreground, _ = util.loadFg(f, **dict(kw, patchshape=patchshape))
            return self._compact[key], numinst, foreground
        if self.pred_file.rstrip("/").endswith(".zarr") and tiling._want_stream(self.pred_file, patchshape, kw):
            aff_key = kw.setdefault("aff_key", "volumes/pred_affs")
            f.raw.add(aff_key)      # a streamed array is never cached whole: the reader hands out the dataset itself,
            arr = f[aff_key]        # to the provider and to a foreground that reads the centre channel
            if len(arr.shape) != 4 or int(arr.shape[0]) != int(np.prod(patchshape)):
                raise NotImplementedError("streaming needs a channels-first (C, Z, Y, X) prediction array")
            for a in "zyx":
                if kw.get("crop_%s_s" % a, 0) or kw.get("crop_%s_e" % a) is not None:
                    raise NotImplementedError("crops are not supported with a streamed prediction")
            numinst = util.maybeLoadNuminst(f, **kw)
            foreground, _ = util.loadFg(f, **dict(kw, patchshape=patchshape))
            logits = kw.get("logits")
            if (aff_key, logits) not in self._provider:
                expit = tiling._logits_in(arr, patchshape) if logits is None else bool(logits)
                self._provider[(aff_key, logits)] = tiling.ZarrProvider(arr, expit=expit)
            return self._provider[(aff_key, logits)], numinst, foreground
        # util.loadAffinities
        if "vote_instances" in f.keys():
            logger.info("%s vote_instances already computed", self.pred_file)
            return None
        pf = util.PredictionFile(f, patchshape=patchshape, **kw)
        key = repr([pf.kw["aff_key"], kw.get("isbiHack")] + [pf._crop("zyx")])
        if key not in self._aff:
            self._aff[key] = self._resident(self._mapped(pf.affinities()))
            # the stored array has served: only its centre channel can be asked for again (the foreground
            # without a fg_key or numinst_key)
            f.keep_channel(pf.kw["aff_key"], int(np.prod(patchshape)) // 2)
        return self._aff[key], pf.numinst(), pf.foreground()[0]

    @staticmethod
    def _mapped(affinities):
        """loadAffinities' last step (utilVoteInstances.py:249-250)"""
        import scipy.special
        if np.min(affinities) < 0 and np.max(affinities) > 1:     # logits
            affinities = scipy.special.expit(affinities)
        return affinities

    def _resident(self, affinities):
        """the host array, or its device copy under the quarter rule"""
        from . import backend
        mode = self.mode
        if mode == "auto":
            import torch
            # a quarter: the bounding-box crop is a second copy, the assembly's pool needs the rest
            fits = torch.cuda.is_available() and affinities.nbytes <= 0.25 * torch.cuda.mem_get_info()[0]
            mode = "device" if fits else "host"
        if mode == "host":
            return affinities
        t0 = time.perf_counter()
        dev = backend.to_device_pred(affinities)
        backend._torch().cuda.synchronize()
        self.times["upload"] += time.perf_counter() - t0
        return dev


# ------------------------------------------------------------------------------------------------
# the sweep
# ------------------------------------------------------------------------------------------------
def select_validation_data(config):
    """run_ppp.py:760-775 without ``validate_on_train``"""
    if config["data"].get("validate_on_train"):
        raise NotImplementedError("[data] validate_on_train is not provided by this repository; unset it")
    data = config["data"]["val_data"]
    if "fold" in config["validation"]:
        data += "_fold" + str(config["validation"]["fold"])
    return data


def eval_params_of(config):
    """run_ppp.py:962-975: the product of ``filterSzs`` and ``res_keys``; a ``filterSz`` other than None is
    refused, as `evaluate` refuses it"""
    if "filterSzs" in config["validation"]:
        filterSzs = config["validation"]["filterSzs"]
    elif "filterSz" in config["evaluation"]:
        filterSzs = [config["evaluation"]["filterSz"]]
    else:
        filterSzs = [None]
    if any(sz is not None for sz in filterSzs):
        raise NotImplementedError("[validation] filterSzs / [evaluation] filterSz is not provided by this "
                                  "repository (evaluate refuses filterSz); unset it")
    res_keys = config["validation"].get("res_keys", [config["evaluation"]["res_key"]])
    return list(named_product(filterSz=filterSzs, res_key=res_keys))


def prediction_folder(pred_folder, checkpoint, n_checkpoints):
    """``<pred_folder>/<checkpoint>/`` when it exists; ``pred_folder`` itself only for a single checkpoint"""
    sub = os.path.join(pred_folder, str(checkpoint))
    if os.path.isdir(sub):
        return sub
    if n_checkpoints != 1:
        raise ValueError("[validation] checkpoints lists %d checkpoints but %s does not exist: predictions "
                         "directly in --pred-folder serve exactly one checkpoint" % (n_checkpoints, sub))
    return pred_folder


def result_exists(config, inst_folder, sample):
    """the rule `label` follows (run_ppp.py:1126-1131)"""
    fmt = config["vote_instances"].get("output_format", "hdf")
    return not config.get("general", {}).get("overwrite", False) and \
        os.path.exists(os.path.join(inst_folder, os.path.basename(sample) + "." + fmt))


def vote_sets(jobs, pred_folder, sample=None):
    """Vote every (config, inst_folder) of ``jobs`` on the predictions of ``pred_folder``, sample-major: a
    sample is opened once and every set that still lacks its result file is voted from it; a sample whose
    result files all exist is never opened."""
    from . import run_ppp
    if not jobs:
        return
    config = jobs[0][0]
    pred_fmt = config["prediction"]["output_format"]
    samples = run_ppp.get_list_samples(pred_folder, pred_fmt, sample)
    cfg = config["vote_instances"]
    if int(cfg.get("batch_2d") or 0) > 1 and not cfg.get("blockwise", False):
        for job_config, inst_folder in jobs:        # (equal shapes voted together, per set: not resident)
            run_ppp.label_batched(copy.deepcopy(job_config), pred_folder, inst_folder, samples)
        return
    for idx, name in enumerate(samples):
        pending = [(c, folder) for c, folder in jobs if not result_exists(c, folder, name)]
        if not pending:
            logger.info("Skipping vote instances for %s. Every result exists!", name)
            continue
        logger.info("validating sample %d/%d: %s (%d sets)", idx, len(samples), name, len(pending))
        with SampleSession(pred_folder, name, pred_fmt) as session:
            for job_config, inst_folder in pending:
                session.vote(job_config, inst_folder)
            logger.info("sample %s: %d sets, load %.2fs, upload %.2fs, vote %.2fs, reads %s", name,
                        session.sets_voted, session.times["load"], session.times["upload"],
                        session.times["vote"], dict(session.reads))


def score_set(config, data, inst_folder, eval_folder, sample=None):
    """the metric of one set: what `run_ppp.evaluate` returns"""
    from . import run_ppp
    return run_ppp.evaluate_folder(config, data, inst_folder, eval_folder, sample)


def validate_checkpoints(config, pred_folder, output_folder, sample=None, val_id=-1):
    """run_ppp.py:919-1051 with ``validate_checkpoint`` :779-853: every checkpoint of ``[validation]
    checkpoints`` times every parameter set (``val_id >= 0``: that index only) times every evaluation parameter
    (``res_keys``) is voted into ``<output_folder>/instanced/<c>/<params_str...>/`` and scored into
    ``<output_folder>/evaluated/<c>/<params_str...>/`` against ``[data] val_data``; ``results.json`` lists
    ``{"checkpoint", "metric", "params"}`` in that order.  Returns (best_checkpoint, best_params): ``np.argmax``
    over the metrics, the first entry wins a tie.

    Prediction and `decode` are NOT run here: the predictions of checkpoint ``c`` are read from
    ``<pred_folder>/<c>/`` when that directory exists, else from ``pred_folder`` itself, which is allowed only when
    exactly one checkpoint is listed.  With ``[evaluation] prediction_only`` nothing is voted: one
    `run_ppp.evaluate_prediction` per checkpoint into ``evaluated/<c>/``, and (None, None) is returned (:926-940).

    A (sample, set) whose result file exists is not voted again unless ``[general] overwrite`` is set.  Inside a
    checkpoint the loop is sample-major (`vote_sets`, `SampleSession`)."""
    import argparse
    from . import run_ppp
    data = select_validation_data(config)
    checkpoints = list(config["validation"]["checkpoints"])
    os.makedirs(output_folder, exist_ok=True)
    if config["evaluation"].get("prediction_only"):
        val_config = copy.deepcopy(config)
        val_config["data"]["test_data"] = data
        for checkpoint in checkpoints:
            folder = prediction_folder(pred_folder, checkpoint, len(checkpoints))
            eval_folder = os.path.join(output_folder, "evaluated", str(checkpoint))
            logger.info("evaluating prediction checkpoint %s", checkpoint)
            metric, ths = run_ppp.evaluate_prediction(
                argparse.Namespace(pred_folder=folder, output_folder=eval_folder, sample=sample), val_config)
            logger.info("%s checkpoint %6s: %s (%s)", config["evaluation"]["metric"], checkpoint, metric, ths)
        return None, None
    eval_params = eval_params_of(config)
    param_sets = param_sets_of(config)
    logger.info("val params %s", param_sets)
    folders = [prediction_folder(pred_folder, c, len(checkpoints)) for c in checkpoints]
    metrics, ckpts, params, results = [], [], [], []
    for checkpoint, ckpt_pred in zip(checkpoints, folders):
        logger.info("validating checkpoint %s", checkpoint)
        runs = []
        for idx, param_set in enumerate(param_sets):
            if val_id >= 0 and val_id != idx:
                continue
            val_config = copy.deepcopy(config)
            for k in param_set:
                val_config["vote_instances"][k] = param_set[k]
            parts = params_str(param_set)
            inst_folder = os.path.join(output_folder, "instanced", str(checkpoint), *parts)
            eval_folder = os.path.join(output_folder, "evaluated", str(checkpoint), *parts)
            os.makedirs(inst_folder, exist_ok=True)
            os.makedirs(eval_folder, exist_ok=True)
            runs.append((param_set, val_config, inst_folder, eval_folder))
        vote_sets([(c, folder) for _, c, folder, _ in runs], ckpt_pred, sample)
        for param_set, val_config, inst_folder, eval_folder in runs:
            for eval_param in eval_params:
                logger.info("eval params %s", eval_param)
                val_config["evaluation"]["res_key"] = eval_param["res_key"]
                val_config["evaluation"]["filterSz"] = eval_param["filterSz"]
                metric = score_set(val_config, data, inst_folder, eval_folder, sample)
                tmp_param_set = copy.deepcopy(param_set)
                tmp_param_set["filterSz"] = eval_param["filterSz"]
                tmp_param_set["res_key"] = eval_param["res_key"]
                metrics.append(metric)
                ckpts.append(checkpoint)
                params.append(tmp_param_set)
                results.append({"checkpoint": checkpoint, "metric": str(metric), "params": tmp_param_set})
                logger.info("%s checkpoint %6s: %.4f (%s)", config["evaluation"]["metric"], checkpoint, metric,
                            tmp_param_set)
    if not metrics:
        raise ValueError("validate: no parameter set to run (val_id = %d of %d sets)" % (val_id, len(param_sets)))
    best = int(np.argmax(metrics))
    logger.info("best checkpoint: %s", ckpts[best])
    logger.info("best params: %s", params[best])
    with open(os.path.join(output_folder, "results.json"), "w") as f:
        json.dump(results, f)
    return ckpts[best], params[best]
