#!/usr/bin/env python3
"""tests/golden/validate/param_sets.json: the reference's own ``get_postprocessing_params``, ``named_params`` and
the folder components of ``validate_checkpoint`` (experiments/run_ppp.py:856-916, :784-787; the module is
imported in place) on small ``[validation]`` sections.  Stubs stand in for what the module imports at its top and
these functions never touch: h5py, zarr, joblib, natsort, toml, git, the PatchPerPix package and
evaluateInstanceSegmentation.  Development container only.

  python tests/golden/gen_golden_validate.py

The file is data only: a list of cases {"name", "validation" (the section, or null), "params_product_list",
"params_zip_list", "vote_instances", "params_zip", "params_product", "sets" (in order), "folders" (the folder
components of every set)}.  The components are produced by executing the reference's own statement (the source
lines :784-787 of ``validate_checkpoint``, which has no function of its own for them) on every set."""
import importlib.util
import inspect
import json
import os
import sys
import textwrap
import types

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "validate")
REF = "/root/reference/experiments"


def load_reference():
    for name in ("h5py", "zarr", "joblib", "natsort", "toml", "git", "PatchPerPix", "PatchPerPix.util",
                 "PatchPerPix.evaluate", "PatchPerPix.vote_instances", "PatchPerPix.visualize",
                 "evaluateInstanceSegmentation"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["joblib"].Parallel = sys.modules["joblib"].delayed = None
    sys.modules["natsort"].natsorted = sorted
    sys.modules["git"].Repo = None
    ppp = sys.modules["PatchPerPix"]
    for sub in ("util", "evaluate", "vote_instances", "visualize"):
        setattr(ppp, sub, sys.modules["PatchPerPix." + sub])
    for name in ("evaluate_patch", "evaluate_numinst", "evaluate_fg"):
        setattr(sys.modules["PatchPerPix.evaluate"], name, None)
    sys.modules["PatchPerPix.visualize"].visualize_patches = None
    sys.modules["PatchPerPix.visualize"].visualize_instances = None
    sys.modules["evaluateInstanceSegmentation"].evaluate_file = None
    sys.modules["evaluateInstanceSegmentation"].summarize_metric_dict = None
    threads = {k: os.environ.get(k) for k in os.environ}
    spec = importlib.util.spec_from_file_location("ppp_ref_run_ppp", os.path.join(REF, "run_ppp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for k in list(os.environ):              # (the module pins the thread counts of its process on import)
        if k not in threads:
            del os.environ[k]
    return mod


def folder_statement(ref):
    """the assignment to ``params_str`` inside the reference's validate_checkpoint, compiled as it stands"""
    lines = inspect.getsource(ref.validate_checkpoint).splitlines()
    start = next(i for i, l in enumerate(lines) if l.strip().startswith("params_str = ["))
    end = next(i for i in range(start, len(lines)) if "for k, v in params.items()]" in lines[i])
    return compile(textwrap.dedent("\n".join(lines[start:end + 1])), "validate_checkpoint:params_str", "exec")


def shipped_validation():
    try:
        import tomllib as toml_reader   # Python >= 3.11
    except ImportError:
        import tomli as toml_reader
    with open(os.path.join(REF, "flylight", "setups", "setup01", "default.toml"), "rb") as f:
        config = toml_reader.load(f)
    return config["validation"], config["vote_instances"]


def main():
    ref = load_reference()
    stmt = folder_statement(ref)
    vi = {"patch_threshold": 0.9, "fc_threshold": 0.7, "mws": True, "skeletonize_foreground": False,
          "numinst_threshs": [0.9, 0.1], "select_patches_for_sparse_data": True}
    two = [[0.9, 0.1], [0.334, 0.334]]
    shipped, shipped_vi = shipped_validation()
    cases = [
        ("product_only", {"params_product": ["mws", "numinst_threshs"], "mws": [False, True], "numinst_threshs": two}, vi),
        ("zip_only", {"params_zip": ["patch_threshold", "fc_threshold"], "patch_threshold": [0.5, 0.8],
                      "fc_threshold": [0.5, 0.8]}, vi),
        ("both", {"params_product": ["mws", "skeletonize_foreground", "numinst_threshs"],
                  "params_zip": ["patch_threshold", "fc_threshold"], "mws": [False, True],
                  "skeletonize_foreground": [True], "numinst_threshs": two, "patch_threshold": [0.5, 0.8],
                  "fc_threshold": [0.5, 0.8]}, vi),
        ("neither", {"checkpoints": [100]}, vi),
        ("older_params_key", {"params": ["mws", "patch_threshold"], "mws": [True, False], "patch_threshold": [0.25, 0.5, 1.0]}, vi),
        ("empty_list_falls_back", {"params_product": ["mws", "numinst_threshs"], "params_zip": ["patch_threshold"],
                                   "mws": [], "numinst_threshs": [], "patch_threshold": []}, vi),
        ("zip_of_unequal_lengths", {"params_zip": ["patch_threshold", "fc_threshold"], "patch_threshold": [0.5, 0.8, 0.9],
                                    "fc_threshold": [0.5, 0.8]}, vi),
        ("floats_bools_tuples_strings", {"params_product": ["sampling", "mws", "output_format", "chunksize"],
                                         "sampling": [1.0, 0.25, 1e-05], "mws": [True], "output_format": ["hdf"],
                                         "chunksize": [[92, 92, 92], [1, 256, 256]]}, vi),
        ("no_section", None, vi),
        ("shipped_default_toml", shipped, shipped_vi),
    ]
    out = []
    for name, validation, test_config in cases:
        if validation is None:
            product_list, zip_list = ["mws"], ["patch_threshold", "fc_threshold"]
        else:
            product_list = validation.get("params_product", validation.get("params", []))
            zip_list = validation.get("params_zip", [])
        params_zip, params_product = ref.get_postprocessing_params(validation, product_list, zip_list, test_config)
        sets = list(ref.named_params(params_zip, params_product))
        folders = []
        for params in sets:
            scope = {"params": params}
            exec(stmt, scope)
            folders.append(scope["params_str"])
        out.append({"name": name, "validation": validation, "params_product_list": product_list,
                    "params_zip_list": zip_list, "vote_instances": test_config, "params_zip": params_zip,
                    "params_product": params_product, "sets": sets, "folders": folders})
        print("%-28s %2d sets  %s" % (name, len(sets), folders[0]))
    by = {c["name"]: c for c in out}
    assert len(by["both"]["sets"]) == 8 and by["both"]["sets"][1]["patch_threshold"] == 0.5 \
        and by["both"]["sets"][4]["patch_threshold"] == 0.8, "the zip is the outer loop"
    assert by["neither"]["sets"] == [{}] and by["neither"]["folders"] == [[]]
    assert by["empty_list_falls_back"]["sets"] == [{"patch_threshold": 0.9, "mws": True, "numinst_threshs": [0.9, 0.1]}]
    assert len(by["zip_of_unequal_lengths"]["sets"]) == 2
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "param_sets.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
