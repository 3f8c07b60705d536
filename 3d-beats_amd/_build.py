"""Builds the package's native libraries for gfx950 with hipcc (cross-compiles without a GPU).  LIBRARIES describes each
one once -- its .so, sources, headers and symbol prefix; everything below, and _lib.py's loader, goes by that table."""
import hashlib
import os
import shutil
import subprocess
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "rdf_hip.hip")
SOURCES = [SRC, os.path.join(HERE, "csrc", "mean_shift_hip.hip"), os.path.join(HERE, "csrc", "points_ops_hip.hip"),
           os.path.join(HERE, "csrc", "tree_train_hip.hip"), os.path.join(HERE, "csrc", "grouping_hip.hip")]
HEADERS = [os.path.join(HERE, "..", "include", "rdf_hip.h"), os.path.join(HERE, "csrc", "rdf_device.hpp"),
           os.path.join(HERE, "csrc", "rdf_host_state.hpp"), os.path.join(HERE, "csrc", "rdf_launch_plan.hpp"),
           os.path.join(HERE, "csrc", "rdf_kernel_util.hpp"), os.path.join(HERE, "csrc", "rdf_modes.hpp")]
SO = os.path.join(HERE, "csrc", "librdf_hip.so")


class Library(NamedTuple):
    key: str
    so: str
    sources: list
    headers: list      # the public header (include/) first
    prefix: str        # of its <prefix>abi_version / <prefix>build_id / <prefix>error_string


# Each library has its own sources and build id, so adding one leaves the others' binaries as they were.
LIBRARIES = {lib.key: lib for lib in (
    Library("hip", SO, SOURCES, HEADERS, "rdf_"),
    # the depth front end, the note state machine behind the fingertip heights, and the depth post-filter in front of both
    Library("frontend", os.path.join(HERE, "csrc", "librdf_frontend.so"),
            [os.path.join(HERE, "csrc", "frontend_hip.hip"), os.path.join(HERE, "csrc", "hand_state_hip.hip"),
             os.path.join(HERE, "csrc", "depth_filter_hip.hip")],
            [os.path.join(HERE, "..", "include", "rdf_frontend.h"), os.path.join(HERE, "csrc", "rdf_kernel_util.hpp")],
            "rdf_frontend_"),
    # glove-colour recordings to training labels, the re-render that augments them, the score of predicted label maps, and
    # labelled frames of the articulated hand, the fit of that hand's pose to a labelled depth frame, and the stereo depth
    # sensor that turns a left and a right render of those frames into what a camera would report, and the refit of a trained
    # forest's leaf distributions on such frames and the pruning of the forest on the same counts, and the forest's posterior:
    # the refit's walk ending in per-pixel class sums, a confidence and a gated label where inference ends in an argmax (these
    # three read the reference-layout forest through rdf_forest_ref.hpp, a header of this library alone: its layout, its flag
    # rule, the one walk and the ancestor's PDF; the walk's feature step -- the offset coordinate and the bounds-checked read
    # -- is that of rdf_device.hpp, the forest and training kernels' header), and the
    # consumer of that confidence: composite weights of a layered stack and the weighted mean shift (soft modes), whose kernel
    # body is the mean shift's own: rdf_modes.hpp is a header of this library and of "hip", and a change to it rebuilds both;
    # and the joint votes, the fourth user of rdf_forest_ref.hpp's walk: offsets towards the joints summed per leaf slot, a vote
    # table made of them, the votes of every hand pixel cast into an accumulator per joint and the accumulator's mode; and the
    # voted fingertips, which choose per tip between the mode's pixel and the vote's and take rdf_modes.hpp's height of it; and
    # the hand's shape, the fifth user of the walk: every hand pixel's shares of its vote pooled per frame, and the held decision
    Library("labels", os.path.join(HERE, "csrc", "librdf_labels.so"),
            [os.path.join(HERE, "csrc", "labels_hip.hip"), os.path.join(HERE, "csrc", "rerender_hip.hip"),
             os.path.join(HERE, "csrc", "score_hip.hip"), os.path.join(HERE, "csrc", "hand_scene_hip.hip"),
             os.path.join(HERE, "csrc", "pose_fit_hip.hip"), os.path.join(HERE, "csrc", "stereo_sensor_hip.hip"),
             os.path.join(HERE, "csrc", "forest_refit_hip.hip"), os.path.join(HERE, "csrc", "forest_prune_hip.hip"),
             os.path.join(HERE, "csrc", "forest_posterior_hip.hip"), os.path.join(HERE, "csrc", "forest_votes_hip.hip"),
             os.path.join(HERE, "csrc", "vote_tips_hip.hip"), os.path.join(HERE, "csrc", "forest_shape_hip.hip"),
             os.path.join(HERE, "csrc", "soft_modes_hip.hip")],
            [os.path.join(HERE, "..", "include", "rdf_labels.h"), os.path.join(HERE, "csrc", "rdf_kernel_util.hpp"),
             os.path.join(HERE, "csrc", "rdf_raster.hpp"), os.path.join(HERE, "csrc", "rdf_device.hpp"),
             os.path.join(HERE, "csrc", "rdf_modes.hpp"), os.path.join(HERE, "csrc", "rdf_forest_ref.hpp")], "rdf_labels_"),
)}

# No -ffast-math, no -fgpu-flush-denormals-to-zero: the fp32 divide must stay IEEE-correct
# and denormals must be kept for bit-exact parity (see rdf_hip.hip header).
HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC",
               "-fno-fast-math", "-ffp-contract=off"]


def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


BUILD_ID_MARKER = b"rdf-build-id:"


def source_id(lib="hip"):
    """16 hex digits of a SHA-256 over everything the library is built from: the sources, the headers, the compiler flags.
    Baked into the library (<prefix>build_id) -- file times say nothing about a .so that travelled with a snapshot."""
    lib = LIBRARIES[lib]
    h = hashlib.sha256()
    for p in sorted(lib.sources + lib.headers, key=os.path.basename):
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    h.update(" ".join(HIPCC_FLAGS).encode())
    return h.hexdigest()[:16]


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


def sources_present(lib="hip"):
    return all(os.path.exists(p) for p in LIBRARIES[lib].sources + LIBRARIES[lib].headers)


def is_stale(lib="hip"):
    """True when the library's .so is missing or was built from other sources than the ones next to it."""
    so = LIBRARIES[lib].so
    if not os.path.exists(so):
        return True
    return sources_present(lib) and built_id(so) != source_id(lib)


def build(force=False, verbose=False):
    """Compile the HIP libraries in-tree (each only when stale).  Returns the path of the main one, librdf_hip.so."""
    for lib in LIBRARIES.values():
        if force or is_stale(lib.key):
            cmd = [hipcc()] + HIPCC_FLAGS + [f'-DRDF_BUILD_ID="{source_id(lib.key)}"', "-o", lib.so + ".tmp"] + lib.sources
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
            os.replace(lib.so + ".tmp", lib.so)
    return SO


if __name__ == "__main__":
    print(build(force=True, verbose=True))
