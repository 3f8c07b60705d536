"""Records tests/golden/frontend_v1.npz: the reference's own `gaussian_kernel(k_size, sigma)` (src/cuda/points_ops.py:8-13)
for the (k, sigma) pairs the front end uses, float32 weights bit for bit.

Runs in the build container only (it loads /root/reference/src/cuda/points_ops.py, which never travels to the GPU box).
The reference module's three package imports (cuda.py_nvcc_utils, engine.buffer, util) need PyCUDA and OpenGL; empty
stand-ins are put into sys.modules for them, since gaussian_kernel uses only numpy and scipy.  The fixture holds data
only: the pairs and the weights.

    python tests/golden/make_frontend_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "frontend_v1.npz")
CASES = [(1, 2.0), (3, 0.5), (3, 1.0), (5, 1.0), (5, 2.0), (5, 3.5), (7, 2.0), (9, 2.0), (11, 4.0), (15, 2.0), (21, 5.0),
         (41, 2.0), (41, 8.0), (41, 13.0)]


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def reference_gaussian_kernel():
    saved = {n: sys.modules.get(n) for n in ("cuda", "cuda.py_nvcc_utils", "engine", "engine.buffer", "util")}
    try:
        _stub("cuda", __path__=[])
        sys.modules["cuda"].py_nvcc_utils = _stub("cuda.py_nvcc_utils")
        _stub("engine", __path__=[])
        sys.modules["engine"].buffer = _stub("engine.buffer", GpuBuffer=object)
        _stub("util", PagelockedCounter=object, make_grid=lambda *a, **k: None)
        spec = importlib.util.spec_from_file_location("ref_points_ops", os.path.join(REF, "src", "cuda", "points_ops.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.gaussian_kernel
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def main():
    gk = reference_gaussian_kernel()
    data = {"k": np.array([k for k, _ in CASES], np.int32), "sigma": np.array([s for _, s in CASES], np.float64)}
    for i, (k, s) in enumerate(CASES):
        w = gk(k, s)
        assert w.dtype == np.float32 and w.shape == (k, k)
        data[f"w{i}"] = w
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
