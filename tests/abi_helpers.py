"""What a header declares and what a shared library exports, for the tests that pin the two to each other."""
import re
import shutil
import subprocess


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(rdf_[a-z0-9_]+)\s*\(", text)))


def exported(so):
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    return sorted({l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("rdf_")})
