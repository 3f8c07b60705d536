"""Mutants of the numpy restatements: a restatement's source is loaded again with one textual replacement, a wrong reading
of a header rule that a kernel could make.  The CPU tests ask of every device case which mutants change one of its outputs
(tests/*_cases.py keep the tables: MUTANTS, KILLS, EQUIVALENT); a mutant that changes none would pass every GPU test.
Nothing here gives a GPU test an expected value: those come from the restatement itself, or from a literal.

An edit is (old, new): `old` must stand in the source exactly once, else the load fails -- a restatement that was reworded
does not lose its mutants silently."""
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def fma(a, b, c):
    """a * b + c with one rounding, EMULATED: the product and the sum in float64, then one rounding to float32.  (A float64
    holds the product of two float32 exactly; the sum is rounded to 53 bits first, so a result within 2^-29 of a float32 tie
    could round the other way than hardware does.  The fma cases store inputs for which this and the separate operations
    differ by a whole snapped unit or stored depth; none depends on such a double rounding.)"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
                + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def load(module, edits=(), **inject):
    """A fresh copy of tests/<module>.py after `edits`, with `inject` put into its namespace after it has run (functions look
    their globals up when called, so an injected name replaces an imported one)."""
    path = os.path.join(HERE, module + ".py")
    with open(path) as fh:
        src = fh.read()
    for old, new in edits:
        found = src.count(old)
        assert found == 1, f"{module}.py holds {old!r} {found} times: the mutant no longer applies"
        assert new != old
        src = src.replace(old, new)
    mod = types.ModuleType(module + "_copy")
    mod.__file__ = path
    mod.__dict__["_fma"] = fma
    exec(compile(src, path, "exec"), mod.__dict__)
    mod.__dict__.update(inject)
    return mod


def same(a, b):
    """Bit for bit, NaN included; tuples and lists element by element."""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return a.tobytes() == b.tobytes()


def changed(a, b):
    """The number of elements in which two tuples of arrays differ (bit patterns: NaN equals NaN)."""
    n = 0
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape
        if x.dtype.kind == "f":
            x, y = x.view(f"u{x.dtype.itemsize}"), y.view(f"u{y.dtype.itemsize}")
        n += int((x != y).sum())
    return n
