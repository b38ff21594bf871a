"""Writes tests/golden/head_post.npz: the reference's own ``postprocess`` (mast3r/catmlp_dpt_head.py:25-39, with
dust3r/heads/postprocess.py:22-55 inside) on the CPU, on the cases of tests/head_cases.py.

Runs only where /root/reference exists (read-only), like make_golden.py. The reference never travels: only the inputs
and its results are committed. Per case (``acc``: the accuracy case, ``lay``: the layout case, ``spc``: the special
values), with the modes of head_cases (depth ('exp', -inf, inf), conf ('exp', 1, inf), desc_conf ('exp', 0, inf),
F = 24, two_confs):
    <case>_out              the input (B, 29, H, W) float32
    <case>_ref32_<key>      the reference's float32 result, key in pts3d, conf, desc, desc_conf
    <case>_ref64_<key>      its float64 result for the same input cast to double

    python tests/golden/make_head_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
sys.path[:0] = [REF, os.path.join(REF, "thirdparty", "mast3r")]

import head_cases as HC  # noqa: E402
from mast3r.catmlp_dpt_head import postprocess as ref_postprocess  # noqa: E402


def run(out, dtype):
    with torch.no_grad():
        res = ref_postprocess(torch.from_numpy(out).to(dtype), HC.DEPTH_MODE, HC.CONF_MODE, desc_dim=HC.F_ACC,
                              desc_mode="norm", two_confs=True, desc_conf_mode=HC.DESC_CONF_MODE)
    assert all(v.dtype == dtype for v in res.values())
    return {k: res[k].numpy() for k in HC.KEYS}


def main():
    cases = dict(acc=HC.accuracy_inputs(HC.ACC_SEED, *HC.ACC_SHAPE), lay=HC.layout_inputs(*HC.LAYOUT_SHAPE),
                 spc=HC.special_inputs())
    data = {}
    for name, out in cases.items():
        data[f"{name}_out"] = out
        for tag, dtype in (("ref32", torch.float32), ("ref64", torch.float64)):
            for k, v in run(out, dtype).items():
                data[f"{name}_{tag}_{k}"] = v
    assert all(np.isfinite(v).all() for k, v in data.items() if k.startswith("acc_"))
    d = HC.norm64(cases["acc"])
    path = os.path.join(HERE, "head_post.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {os.path.getsize(path)} bytes; accuracy case d in [{d.min():.3g}, {d.max():.3g}]")
    _, e_ref = HC.bounds(data)
    print("e_ref (2^-24):", {k: round(v, 2) for k, v in e_ref.items()})


if __name__ == "__main__":
    main()
