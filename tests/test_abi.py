"""The C-ABI libraries build for gfx950, load, and export exactly the symbols their headers declare.  What holds for each
library alike is tested once, for every entry of _build.LIBRARIES; what only one library has (sizes, return codes, structs)
is with that library's tests.  No compute calls (no GPU here)."""
import ctypes
import os
import shutil
import subprocess
from importlib import import_module

import pytest

from abi_helpers import declared, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = ("hip", "frontend", "labels")
C99 = ["-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]


def _declared():
    return declared(os.path.join(ROOT, "include", "rdf_hip.h"))


def _modules():
    return import_module("3d-beats_amd._build"), import_module("3d-beats_amd._lib")


def _copy_with_another_id(build, so, tmp_path):
    """The same library with another id baked in (as if built before the last edit of a kernel)."""
    blob = bytearray(open(so, "rb").read())
    at = blob.find(build.BUILD_ID_MARKER) + len(build.BUILD_ID_MARKER)
    assert at >= len(build.BUILD_ID_MARKER) and blob.count(build.BUILD_ID_MARKER) == 1
    blob[at:at + 16] = b"0123456789abcdef"
    stale = tmp_path / os.path.basename(so).replace(".so", "_stale.so")
    stale.write_bytes(bytes(blob))
    assert build.built_id(str(stale)) == "0123456789abcdef"
    return str(stale)


def test_header_declares_the_three_reference_kernels():
    names = _declared()
    for n in ("rdf_eval_forest", "rdf_eval_tree", "rdf_composite"):
        assert n in names


def test_library_builds_and_exports_every_declared_symbol(rdf):
    build = import_module("3d-beats_amd._build")
    so = build.build()
    assert os.path.exists(so)
    lib = ctypes.CDLL(so)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/rdf_hip.h but not exported"


def test_binding_table_matches_header(rdf):
    _lib = import_module("3d-beats_amd._lib")
    assert sorted(_lib.SIGNATURES) == _declared()
    lib = _lib.load()
    assert lib.rdf_abi_version() == _lib.ABI_VERSION
    # two tables per heap slot (16-byte hot record, PDF rows); up to four classes: the 64-byte records of the deepest level and a
    # 64-byte trailer; up to eight classes and five levels or more: the deep blocks (128-byte aligned), a zero line and a
    # 128-byte trailer; last: the 128-byte info block
    def deep(T, D, last):       # lines: three-level blocks rooted on levels R0 - 3, R0 - 6, ... >= 0, then the last blocks
        r0 = D - last
        return T * (((1 << r0) - (1 << (r0 % 3))) // 7) + (T << r0) + 2

    def up128(n):
        return (n + 127) & ~127
    assert lib.rdf_forest_packed_bytes(4, 20, 4) == up128((4 << 20) * (16 + 32) + (4 << 19) * 64 + 64) + deep(4, 20, 2) * 128 + 128
    assert lib.rdf_forest_packed_bytes(2, 1, 3) == up128((2 << 1) * (16 + 32)) + 128
    assert lib.rdf_forest_packed_bytes(2, 4, 3) == up128((2 << 4) * (16 + 32) + (2 << 3) * 64 + 64) + 128
    assert lib.rdf_forest_packed_bytes(3, 10, 5) == up128((3 << 10) * (16 + 64)) + deep(3, 10, 1) * 128 + 128
    assert lib.rdf_forest_packed_bytes(3, 10, 9) == up128((3 << 10) * (16 + 96)) + 128
    assert lib.rdf_forest_packed_bytes(0, 10, 4) == 0 and lib.rdf_forest_packed_bytes(4, 0, 4) == 0
    # deep blocks for forests of 5 to 24 levels and up to eight classes, whatever the number of trees
    lib.rdf_forest_packed_bytes.restype, lib.rdf_forest_packed_bytes.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    for T in (6, 8):
        assert lib.rdf_forest_packed_bytes(T, 24, 4) == up128((T << 24) * (16 + 32) + (T << 23) * 64 + 64) + deep(T, 24, 2) * 128 + 128
    assert lib.rdf_forest_packed_bytes(2, 25, 4) == up128((2 << 25) * (16 + 32) + (2 << 24) * 64 + 64) + 128
    assert lib.rdf_forest_packed_bytes(8, 22, 4) == up128((8 << 22) * (16 + 32) + (8 << 21) * 64 + 64) + deep(8, 22, 2) * 128 + 128
    assert b"2^31" in lib.rdf_error_string(-3)


def test_the_library_table_is_these_three(rdf):
    build, _lib = _modules()
    assert tuple(build.LIBRARIES) == tuple(_lib.BINDINGS) == LIBS
    assert [build.LIBRARIES[k].prefix for k in LIBS] == ["rdf_", "rdf_frontend_", "rdf_labels_"]
    assert build.LIBRARIES["hip"][1:4] == (build.SO, build.SOURCES, build.HEADERS)
    assert len({build.LIBRARIES[k].so for k in LIBS}) == 3


@pytest.mark.parametrize("name", LIBS)
def test_library_binding_header_and_sources_agree(name, rdf):
    """Binding table == the header's declarations == the .so's exported rdf_* symbols, none of them another library's; the
    ABI number is the binding's; the id baked into the file is the one of the sources next to it."""
    build, _lib = _modules()
    build.build()
    rec = build.LIBRARIES[name]
    names = declared(rec.headers[0])
    assert sorted(_lib.BINDINGS[name][1]) == names
    assert exported(rec.so) == names
    for what in ("abi_version", "build_id", "error_string"):
        assert rec.prefix + what in names
    for other in LIBS:
        if other != name:
            assert not set(names) & (set(_lib.BINDINGS[other][1]) | set(exported(build.LIBRARIES[other].so))), other
    lib = _lib.load(name)
    assert lib is _lib.load(name)
    assert getattr(lib, rec.prefix + "abi_version")() == _lib.BINDINGS[name][0]
    got = getattr(lib, rec.prefix + "build_id")().decode()
    assert len(got) == 16 and got == build.source_id(name) == build.built_id(rec.so)
    assert build.sources_present(name) and not build.is_stale(name)


def test_the_shared_modes_body_is_in_the_build_id_of_both_its_libraries(rdf, tmp_path, monkeypatch):
    """csrc/rdf_modes.hpp is compiled into librdf_hip.so (k_mean_shift_fused) and librdf_labels.so (k_weighted_modes): it is a
    header of both, and a change to it changes both ids -- a librdf_hip.so from before the change would otherwise pass the
    build-id check.  (On a copy of the sources: nothing in the tree is touched.)"""
    users, in_tree, touched = _ids_after_touching("rdf_modes.hpp", tmp_path, monkeypatch)
    assert users == ["hip", "labels"]
    assert touched["hip"] != in_tree["hip"] and touched["labels"] != in_tree["labels"]
    assert touched["frontend"] == in_tree["frontend"]


def _ids_after_touching(header, tmp_path, monkeypatch):
    """The libraries that list `header`, every library's id in the tree, and every library's id on a copy of the sources in
    which each user's copy of `header` has a line more."""
    build, _ = _modules()
    users = [name for name in LIBS if header in map(os.path.basename, build.LIBRARIES[name].headers)]
    in_tree = {name: build.source_id(name) for name in LIBS}
    copies = {}
    for name in LIBS:
        rec = build.LIBRARIES[name]
        os.mkdir(tmp_path / name)
        copies[name] = rec._replace(sources=[shutil.copy(p, tmp_path / name) for p in rec.sources],
                                    headers=[shutil.copy(p, tmp_path / name) for p in rec.headers])
    monkeypatch.setattr(build, "LIBRARIES", copies)
    assert {name: build.source_id(name) for name in LIBS} == in_tree
    for name in users:
        with open(tmp_path / name / header, "a") as f:
            f.write("// touched\n")
    return users, in_tree, {name: build.source_id(name) for name in LIBS}


def test_the_reference_layout_forest_header_is_in_the_build_id_of_the_labels_library_alone(rdf, tmp_path, monkeypatch):
    """csrc/rdf_forest_ref.hpp holds the walk of the refit, the pruning and the posterior, all of librdf_labels.so: the three
    sources include it, it is a header of that library and of no other, and a change to it changes that id and leaves the
    forest evaluation's and the front end's as they were."""
    build, _ = _modules()
    for src in ("forest_refit_hip.hip", "forest_prune_hip.hip", "forest_posterior_hip.hip"):
        path, = [p for p in build.LIBRARIES["labels"].sources if os.path.basename(p) == src]
        assert '#include "rdf_forest_ref.hpp"' in open(path).read(), src
    users, in_tree, touched = _ids_after_touching("rdf_forest_ref.hpp", tmp_path, monkeypatch)
    assert users == ["labels"]
    assert touched["labels"] != in_tree["labels"]
    assert touched["hip"] == in_tree["hip"] and touched["frontend"] == in_tree["frontend"]


@pytest.mark.parametrize("name", LIBS)
def test_code_object_targets_gfx950(name, rdf):
    build = import_module("3d-beats_amd._build")
    build.build()
    blob = open(build.LIBRARIES[name].so, "rb").read()
    assert b"gfx950" in blob


def test_code_object_stays_small(rdf, tmp_path):
    """Every instantiation of the forest kernel costs compile time and code size; kForestKernels in rdf_launch_plan.hpp lists
    the ones launches really take.  Fewer than 75 of them (16 walk the deep blocks, 4 count visits and lines), and a library under 1.9 MB."""
    import shutil
    import subprocess
    so = import_module("3d-beats_amd._build").build()
    assert os.path.getsize(so) < 1_900_000, os.path.getsize(so)
    objdump = shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump")
    local = tmp_path / "lib.so"
    shutil.copy(so, local)
    subprocess.check_call([objdump, "--offloading", str(local)], cwd=tmp_path, stdout=subprocess.DEVNULL)
    kernels = set()
    for f in os.listdir(tmp_path):
        if "gfx950" in f:
            out = subprocess.run([objdump, "-t", str(tmp_path / f)], capture_output=True, text=True).stdout
            kernels |= {l.split()[-1] for l in out.splitlines()
                        if "k_eval_forest" in l and " F " in l and not l.split()[-1].endswith(".kd")}
    assert 0 < len(kernels) < 75, len(kernels)


def test_no_gpu_means_loud_failure_not_cpu_fallback(rdf):
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    prev = rdf.set_runtime(None)
    try:
        with pytest.raises(rdf.RdfError):
            rdf.get_runtime()
        with pytest.raises(rdf.RdfError):
            rdf.DecisionTreeEvaluator()
    finally:
        rdf.set_runtime(prev)


def test_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "3d-beats_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "librdf_oracle" not in src, f


@pytest.mark.parametrize("name", LIBS)
def test_header_is_plain_c(name, rdf, tmp_path):
    """A public header is what a C (or cgo / JNI / N-API) binding would include: it must compile as pedantic C99, on its own."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    rec = import_module("3d-beats_amd._build").LIBRARIES[name]
    src = tmp_path / "t.c"
    src.write_text(f'#include "{os.path.basename(rec.headers[0])}"\n'
                   f'int main(void) {{ return {rec.prefix}abi_version() > 0 ? 0 : 1; }}\n')
    subprocess.check_call([gcc] + C99 + [str(src)])


def test_headers_are_plain_c_together(rdf, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    recs = import_module("3d-beats_amd._build").LIBRARIES.values()
    src = tmp_path / "t.c"
    src.write_text("".join(f'#include "{os.path.basename(r.headers[0])}"\n' for r in recs)
                   + "int main(void) { return " + " && ".join(f"{r.prefix}abi_version() > 0" for r in recs) + " ? 0 : 1; }\n")
    subprocess.check_call([gcc] + C99 + [str(src)])


@pytest.mark.gpu
def test_plain_c_consumer_of_the_shared_library(rdf, gpu_runtime, tmp_path):
    """examples/eval_forest.c, built with gcc against librdf_hip.so and the HIP runtime's C API, evaluates a one-node
    forest and checks the labels itself."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(rdf.library_path())
    exe = tmp_path / "eval_forest_example"
    subprocess.check_call([gcc, "-std=c99", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(root, "include"),
                           "-I", "/opt/rocm/include", os.path.join(root, "examples", "eval_forest.c"),
                           "-L", libdir, "-l:librdf_hip.so", "-L", "/opt/rocm/lib", "-lamdhip64",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "PASS" in out.stdout, (out.returncode, out.stdout, out.stderr)


@pytest.mark.parametrize("name", LIBS)
def test_a_library_built_from_other_sources_is_refused(name, rdf, tmp_path, monkeypatch):
    """Build identity: each library carries a hash of the sources it was built from (<prefix>build_id); the binding recomputes
    it from csrc/ + include/ and refuses a mismatch -- a library with today's ABI number and yesterday's kernels passes every
    other check (the .so is git-ignored and travels to the GPU box with the snapshot; file times mean nothing there)."""
    build, _lib = _modules()
    monkeypatch.delenv("RDF_HIP_LIBRARY", raising=False)
    monkeypatch.delenv("RDF_ALLOW_STALE_LIBRARY", raising=False)
    build.build()
    rec = build.LIBRARIES[name]
    assert build.built_id(rec.so) == build.source_id(name) and not build.is_stale(name)
    if name == "hip":
        assert build.built_id() == build.source_id() and not build.is_stale()
    lib = ctypes.CDLL(rec.so)
    getattr(lib, rec.prefix + "build_id").restype = ctypes.c_char_p
    assert _lib.check_build_id(lib, rec.so, name) == build.source_id(name)
    stale = _copy_with_another_id(build, rec.so, tmp_path)
    old = ctypes.CDLL(stale)
    getattr(old, rec.prefix + "build_id").restype = ctypes.c_char_p
    with pytest.raises(_lib.RdfError, match="built from other sources"):
        _lib.check_build_id(old, stale, name)
    # ... and load() is what refuses it, when that file is the library's
    monkeypatch.setattr(_lib, "_loaded", {})
    monkeypatch.setitem(build.LIBRARIES, name, rec._replace(so=stale))
    with pytest.raises(_lib.RdfError, match="built from other sources"):
        _lib.load(name)
    monkeypatch.setenv("RDF_ALLOW_STALE_LIBRARY", "1")
    with pytest.warns(UserWarning, match="built from other sources"):
        _lib.check_build_id(old, stale, name)
    with pytest.warns(UserWarning, match="built from other sources"):
        assert getattr(_lib.load(name), rec.prefix + "build_id")() == b"0123456789abcdef"
    monkeypatch.delenv("RDF_ALLOW_STALE_LIBRARY")
    monkeypatch.setitem(build.LIBRARIES, name, rec)
    # is_stale() sees an edited source without looking at file times
    monkeypatch.setattr(build, "HIPCC_FLAGS", build.HIPCC_FLAGS + ["-DSOMETHING_ELSE"])
    assert build.is_stale(name)


def test_rdf_hip_library_redirects_the_main_library_only(rdf, tmp_path, monkeypatch):
    """RDF_HIP_LIBRARY is for timing other builds of the forest kernel: it names the file load() opens as the main library and
    exempts it from the build-id check; the front-end and labels libraries cannot be pointed elsewhere and stay checked."""
    build, _lib = _modules()
    monkeypatch.delenv("RDF_ALLOW_STALE_LIBRARY", raising=False)
    build.build()
    alt = _copy_with_another_id(build, build.SO, tmp_path)
    monkeypatch.setenv("RDF_HIP_LIBRARY", alt)
    monkeypatch.setattr(_lib, "_loaded", {})
    assert _lib.library_path() == _lib.library_path("hip") == alt
    lib = _lib.load()
    assert lib.rdf_build_id() == b"0123456789abcdef" and lib.rdf_abi_version() == _lib.ABI_VERSION
    assert alt in open("/proc/self/maps").read()
    for name in ("frontend", "labels"):
        rec = build.LIBRARIES[name]
        assert _lib.library_path(name) == rec.so
        assert getattr(_lib.load(name), rec.prefix + "build_id")().decode() == build.source_id(name)
        stale = _copy_with_another_id(build, rec.so, tmp_path)
        monkeypatch.setitem(build.LIBRARIES, name, rec._replace(so=stale))
        monkeypatch.setattr(_lib, "_loaded", {})
        with pytest.raises(_lib.RdfError, match="built from other sources"):
            _lib.load(name)


@pytest.mark.parametrize("name", LIBS)
def test_a_missing_library_names_its_path_and_the_build_command(name, rdf, tmp_path, monkeypatch):
    build, _lib = _modules()
    monkeypatch.delenv("RDF_HIP_LIBRARY", raising=False)
    gone = str(tmp_path / os.path.basename(build.LIBRARIES[name].so))
    monkeypatch.setitem(build.LIBRARIES, name, build.LIBRARIES[name]._replace(so=gone))
    monkeypatch.setattr(_lib, "_loaded", {})
    with pytest.raises(_lib.RdfError, match="is missing: build it first") as e:
        _lib.load(name)
    assert gone in str(e.value) and "python __graft_entry__.py build" in str(e.value)
