#!/usr/bin/env python3
"""Writes ``tests/golden/law_surface.npz``: the answers of ``tests/law_surface.survey`` (descriptor fields, layouts, refusals,
parameter validation, initial state, two increments per accepted layout at N = 65) together with the inputs they were given.

Record it from the library of the PARENT of a change to the host side, never from the code under test: build the parent's
``csrc`` from ``git archive <parent> dolfinx_materials_amd/csrc include`` in a scratch directory and run, on a GPU,

    DXM_LIB_PATH=<scratch>/dolfinx_materials_amd/libdxmat.so python tests/golden/make_law_surface.py [out.npz]"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from dolfinx_materials_amd import _lib  # noqa: E402
import law_surface as ls  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "law_surface.npz")
    inputs = ls.make_inputs()
    meta, arrays = ls.survey(_lib.load(), inputs)
    for law, incs in inputs.items():
        for k, g in enumerate(incs):
            arrays[f"law{law}/input{k}"] = g
    np.savez_compressed(out, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
    for law, m in meta["laws"].items():
        print(law, m["kernel_name"], {k: [(s["n_plastic"], s["max_local_iters"]) for s in v] for k, v in m["stats"].items()})
    print(f"{_lib.LIB_PATH} -> {out}: {len(arrays)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
