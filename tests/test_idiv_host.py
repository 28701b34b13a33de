"""csrc/idiv.h — the chain launch's divide-free index arithmetic — against the plain division, on the host.

tests/host/idiv_check.cpp is a stand-alone program: it sweeps every divisor and dividend the kernels can meet (state
sizes 1 .. 90, action sizes 1 .. 21 within the layer-0 fan-in limit, the narrow tiles' columns, the tiles' coordinates)
and is built here with AddressSanitizer and UndefinedBehaviorSanitizer; no Python process loads sanitized code."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "host" / "idiv_check.cpp"


def _cxx():
    for cand in ("g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cand) or (cand if Path(cand).exists() else None)
        if path:
            return path
    return None


def test_idiv_matches_the_division_under_the_sanitizers(tmp_path):
    cxx = _cxx()
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "idiv_check"
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, str(SRC), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "idiv_check: ok" in run.stdout
    # the multipliers the program printed are idiv.h's own row_div_magic(d): floor(2^20 / d) + 1, the value the host
    # writes into ChainArgs and launch_ddpg_chain compares before it launches
    magics = dict(tuple(map(int, ln.split()[1:])) for ln in run.stdout.splitlines() if ln.startswith("magic "))
    assert sorted(magics) == list(range(1, 257))
    assert all(m == (1 << 20) // d + 1 for d, m in magics.items())
