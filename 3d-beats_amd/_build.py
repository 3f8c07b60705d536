"""Builds csrc/librdf_hip.so, csrc/librdf_frontend.so and csrc/librdf_labels.so for gfx950 with hipcc (cross-compiles
without a GPU)."""
import hashlib
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "rdf_hip.hip")
SOURCES = [SRC, os.path.join(HERE, "csrc", "mean_shift_hip.hip"), os.path.join(HERE, "csrc", "points_ops_hip.hip"),
           os.path.join(HERE, "csrc", "tree_train_hip.hip"), os.path.join(HERE, "csrc", "grouping_hip.hip")]
HEADERS = [os.path.join(HERE, "..", "include", "rdf_hip.h"), os.path.join(HERE, "csrc", "rdf_device.hpp")]
SO = os.path.join(HERE, "csrc", "librdf_hip.so")
# the depth front end (include/rdf_frontend.h): a library of its own, with its own sources and build id
FRONTEND_SOURCES = [os.path.join(HERE, "csrc", "frontend_hip.hip")]
FRONTEND_HEADERS = [os.path.join(HERE, "..", "include", "rdf_frontend.h")]
FRONTEND_SO = os.path.join(HERE, "csrc", "librdf_frontend.so")
# glove-colour recordings to training labels (include/rdf_labels.h): the third library, on the same terms
LABELS_SOURCES = [os.path.join(HERE, "csrc", "labels_hip.hip")]
LABELS_HEADERS = [os.path.join(HERE, "..", "include", "rdf_labels.h")]
LABELS_SO = os.path.join(HERE, "csrc", "librdf_labels.so")

# No -ffast-math, no -fgpu-flush-denormals-to-zero: the fp32 divide must stay IEEE-correct
# and denormals must be kept for bit-exact parity (see rdf_hip.hip header).
HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC",
               "-fno-fast-math", "-ffp-contract=off"]


def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


BUILD_ID_MARKER = b"rdf-build-id:"


def source_id(files=None):
    """16 hex digits of a SHA-256 over everything the library is built from: the sources, the headers, the compiler flags.
    Baked into the library (rdf_build_id) -- file times say nothing about a .so that travelled with a snapshot.
    `files`: another library's sources and headers (frontend_source_id)."""
    h = hashlib.sha256()
    for p in sorted(files or SOURCES + HEADERS, key=os.path.basename):
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    h.update(" ".join(HIPCC_FLAGS).encode())
    return h.hexdigest()[:16]


def frontend_source_id():
    return source_id(FRONTEND_SOURCES + FRONTEND_HEADERS)


def labels_source_id():
    return source_id(LABELS_SOURCES + LABELS_HEADERS)


def built_id(path=None):
    """The id baked into a built library, read from the file (no dlopen); None if there is none."""
    try:
        with open(path or SO, "rb") as f:
            blob = f.read()
    except OSError:
        return None
    at = blob.find(BUILD_ID_MARKER)
    if at < 0:
        return None
    return blob[at + len(BUILD_ID_MARKER):at + len(BUILD_ID_MARKER) + 16].decode("ascii", "replace")


def sources_present(files=None):
    return all(os.path.exists(p) for p in (files or SOURCES + HEADERS))


def is_stale():
    """True when csrc/librdf_hip.so is missing or was built from other sources than the ones next to it."""
    if not os.path.exists(SO):
        return True
    return sources_present() and built_id() != source_id()


def frontend_is_stale():
    """The same for csrc/librdf_frontend.so."""
    if not os.path.exists(FRONTEND_SO):
        return True
    return sources_present(FRONTEND_SOURCES + FRONTEND_HEADERS) and built_id(FRONTEND_SO) != frontend_source_id()


def labels_is_stale():
    """The same for csrc/librdf_labels.so."""
    if not os.path.exists(LABELS_SO):
        return True
    return sources_present(LABELS_SOURCES + LABELS_HEADERS) and built_id(LABELS_SO) != labels_source_id()


def _compile(so, sources, sid, verbose):
    cmd = [hipcc()] + HIPCC_FLAGS + [f'-DRDF_BUILD_ID="{sid}"', "-o", so + ".tmp"] + sources
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(so + ".tmp", so)


def build(force=False, verbose=False):
    """Compile the three HIP libraries in-tree (each only when stale).  Returns the path of the main one, librdf_hip.so."""
    if force or is_stale():
        _compile(SO, SOURCES, source_id(), verbose)
    if force or frontend_is_stale():
        _compile(FRONTEND_SO, FRONTEND_SOURCES, frontend_source_id(), verbose)
    if force or labels_is_stale():
        _compile(LABELS_SO, LABELS_SOURCES, labels_source_id(), verbose)
    return SO


if __name__ == "__main__":
    print(build(force=True, verbose=True))
