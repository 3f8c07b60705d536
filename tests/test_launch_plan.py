"""The forest launch's plan (3d-beats_amd/csrc/rdf_launch_plan.hpp: geometry, LDS layout, table sizes, which kernel a launch
takes) is arithmetic and needs no GPU: tests/launch_plan_main.cpp checks it as a stand-alone program under the address +
undefined-behaviour sanitizers.  The header must compile without HIP, as it stands."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "3d-beats_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_launch_plan_under_sanitizer(tmp_path):
    exe = str(tmp_path / "launch_plan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", CSRC, "-o", exe, os.path.join(HERE, "launch_plan_main.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    # (the knobs read the RDF_* environment: the program sets what it sweeps through the Knob objects and nothing else is set)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RDF_")}
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "launch plan ok" in run.stdout
