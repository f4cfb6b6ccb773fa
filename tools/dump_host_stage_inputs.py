#!/usr/bin/env python3
"""Development aid: run one flylight140_p7 step with the shipped flags on the GPU and save what the
two host stages (set-cover thinning, mutex watershed) receive and return, so that they can be
profiled / re-implemented off the GPU box.  Writes host_stage_inputs.npz into the output folder
(PPP_OUT_DIR, default out/) and, for the watershed's host loop alone (ppp_host_mws_sorted),
mws_edges_<workload>.npz: the sorted edge list eu / ev (bit 31 of ev = attractive), n_nodes, the
labels and the ids issued -- tools/time_mws.py --edges takes that file."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from patchperpix_amd import backend, flags  # noqa: E402
from patchperpix_amd.vote_instances import vote_instances as vi  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "flylight140_p7"
shape, ps, cell = bench.WORKLOADS[name]
kw = dict(flags.FLYLIGHT)
P = backend.make_params(shape, ps, **kw)
labels = bench.device_labels(torch, shape, cell, seed=0)
pred = backend.synth_pred(labels, P, seed=0, f16=True)
fg = (labels != 0).cpu().numpy()
saved = {}
orig_thin, orig_mws = backend.host_thin_cover, backend.host_mws
orig_edges = backend.mws_edges_device


def thin(mask, patchshape, sel_lin, bits):
    t0 = time.perf_counter()
    keep = orig_thin(mask, patchshape, sel_lin, bits)
    saved.update(thin_mask=np.packbits(mask.astype(bool)), thin_sel_lin=sel_lin, thin_bits=bits,
                 thin_keep=keep, thin_seconds=time.perf_counter() - t0)
    return keep


def mws(pairs, aff, shp):
    t0 = time.perf_counter()
    out = orig_mws(pairs, aff, shp)
    saved.update(mws_pairs=np.asarray(pairs).astype(np.uint8), mws_aff=aff, mws_nodes=out[0],
                 mws_labels=out[1], mws_n_labels=out[2], mws_seconds=time.perf_counter() - t0)
    return out


def edges(rows, aff, nodes, P_):
    eu, ev = orig_edges(rows, aff, nodes, P_)
    k = int(nodes.shape[0])
    lab = np.zeros((k,), dtype=np.int32)
    times = []
    for _ in range(5):                      # the loop on this host, the list warm after the first
        t0 = time.perf_counter()
        issued = int(backend.lib().ppp_host_mws_sorted(backend._np_ptr(eu), backend._np_ptr(ev), len(eu), k,
                                                       backend._np_ptr(lab)))
        times.append(1e3 * (time.perf_counter() - t0))
    saved_edges.update(eu=eu.copy(), ev=ev.copy(), n_nodes=np.int64(k), labels=lab, issued=np.int64(issued),
                       loop_ms=np.array(times))
    return eu, ev


saved_edges = {}
backend.host_thin_cover, backend.host_mws, backend.mws_edges_device = thin, mws, edges
inst, _ = vi.to_instance_seg(pred, fg.copy(), fg.copy(), fg.astype(np.uint8), ps, **kw)
print("instances", len(np.unique(inst)) - 1, "thin s", saved.get("thin_seconds"), "mws s", saved.get("mws_seconds"))
OUT = os.path.join(ROOT, os.environ.get("PPP_OUT_DIR", "out"))
os.makedirs(OUT, exist_ok=True)
np.savez_compressed(os.path.join(OUT, "host_stage_inputs.npz"), shape=np.array(shape),
                    patchshape=np.array(ps), instances=inst, **saved)
if saved_edges:
    print("mws edges", len(saved_edges["eu"]), "nodes", int(saved_edges["n_nodes"]), "ids issued",
          int(saved_edges["issued"]), "loop ms", " ".join("%.2f" % t for t in saved_edges["loop_ms"]))
    np.savez(os.path.join(OUT, "mws_edges_%s.npz" % name), **saved_edges)
