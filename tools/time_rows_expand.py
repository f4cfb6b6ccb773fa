#!/usr/bin/env python3
"""Times ppp_rows_expand (csrc/ppp_rows.hip) against the torch way of filling a box from rows,
``out.zero_(); out.reshape(C, -1)[:, dst] = rows.t()`` -- the fallback line of decode.decode_into --
on the same rows and mask, asserts that both give the same bits, and prints one JSON line per case.

Box: --side^3 (default 128) at 7^3 float16, foreground 3 % and 90 % (uniformly random voxels).  Times
are between HIP events on the stream, best of --reps after a warm-up; `rate_tb_s` is
(rows bytes read + box bytes written) / time of the kernel -- next to 6.0-6.2 TB/s measured for plain
one-dword-per-lane stores on this chip into tables of 75-302 MB; `fill_ms` / `fill_rate_tb_s` is
`out.zero_()` on the same box, the store-only floor of either way at THIS size.

    python tools/time_rows_expand.py [--side 128] [--fg 0.03 0.9] [--reps 3] [--dtype float16]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best_ms(fn, reps):
    import torch
    fn()                                        # warm-up
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None or ms < best else best
    return best


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=128)
    ap.add_argument("--fg", type=float, nargs="+", default=[0.03, 0.9])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16", "float32"])
    ap.add_argument("--channels", type=int, default=343)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_rows_expand.py needs a GPU: a timing without one says nothing")
    from patchperpix_amd import backend
    dtype = getattr(torch, args.dtype)
    iv = torch.int32 if dtype == torch.float32 else torch.int16
    n, C = args.side, args.channels
    shape, box = (n, n, n), (0, n, 0, n, 0, n)
    g = torch.Generator(device="cuda").manual_seed(0)
    for frac in args.fg:
        mask = torch.rand(shape, generator=g, device="cuda") < frac
        index, n_rows = backend.rows_index_build(mask)
        rows = torch.randn((n_rows, C), generator=g, device="cuda").to(dtype)
        dst = torch.nonzero(mask.reshape(-1)).reshape(-1)
        out_k = torch.empty((C,) + shape, dtype=dtype, device="cuda")
        out_t = torch.empty_like(out_k)

        def kernel():
            backend.rows_expand(rows, index, shape, box, out=out_k)

        def torch_form():
            out_t.zero_()
            out_t.reshape(C, -1)[:, dst] = rows.t()
        ms_k, ms_t = best_ms(kernel, args.reps), best_ms(torch_form, args.reps)
        assert torch.equal(out_k.view(iv), out_t.view(iv)), "the kernel and the torch form differ"
        # what this device gives a plain fill of the same box (the store-only floor of either way)
        ms_fill = best_ms(lambda: out_t.zero_(), args.reps)
        moved = rows.numel() * rows.element_size() + out_k.numel() * out_k.element_size()
        print(json.dumps({"box": list(shape), "channels": C, "dtype": args.dtype, "foreground": frac, "rows": n_rows,
                          "equal": True, "kernel_ms": round(ms_k, 3), "torch_ms": round(ms_t, 3),
                          "torch_over_kernel": round(ms_t / ms_k, 2), "bytes_moved_gb": round(moved / 1e9, 3),
                          "rate_tb_s": round(moved / (ms_k * 1e-3) / 1e12, 3), "plain_store_rate_tb_s": "6.0-6.2",
                          "fill_ms": round(ms_fill, 3),
                          "fill_rate_tb_s": round(out_k.numel() * out_k.element_size() / (ms_fill * 1e-3) / 1e12, 3)}),
              flush=True)
        del out_k, out_t, rows
    return 0


if __name__ == "__main__":
    sys.exit(main())
