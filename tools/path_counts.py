"""Static instruction mix of the chain kernels, per barrier-delimited segment (no GPU needed):

   python tools/path_counts.py [--asm FILE.s] [--filter NAME] [--top N]

Without --asm the device assembly of oprl_amd/csrc/fused_ddpg.hip is produced with hipcc -S and the flags of
oprl_amd/build.py.  For every k_ddpg_chain<P> the tool prints the kernel's register counts and code bytes (the
.amdhsa_ / metadata lines of the assembly) and one row per segment — the instructions between two s_barrier in TEXT
order — with the instructions sorted into classes by their generic prefix only:

   mfma   v_mfma*            valu   other v_*          sload  scalar loads (s_load* / s_buffer_load*)
   wait   s_waitcnt*         br     s_branch / s_cbranch* / s_setpc / s_swappc / s_call
   salu   other s_*          lds    ds_*               vmem   global_* / buffer_* / flat_* / scratch_*

It also counts the run-time integer divisions: hipcc expands `n / d` with a run-time d around one v_rcp_iflag_f32 (an
instruction it emits for nothing else), so the occurrences of that generic vector op are the division sequences.

Text order is not execution order: a segment is a stretch of the code, and a wave runs through the stretches its role
takes.  What the table shows is where the non-arithmetic instructions sit between the stretches that hold the MFMAs."""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
import tempfile
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CLASSES = ["mfma", "valu", "sload", "wait", "br", "salu", "lds", "vmem", "other"]


def classify(op: str) -> str:
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "sload"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call")):
        return "br"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def demangle(names: list[str]) -> dict[str, str]:
    for tool in ("llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool, *names], capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def device_asm() -> str:
    sys.path.insert(0, str(ROOT))
    from oprl_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "fused_ddpg.s"
        cmd = [b._hipcc(), *b.CFLAGS, "--cuda-device-only", "-S", str(b.CSRC / "fused_ddpg.hip"), "-o", str(out)]
        subprocess.run(cmd, check=True, cwd=str(b.CSRC))
        return out.read_text()


INSTR = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")


def kernels(text: str) -> dict[str, dict]:
    """name -> {"body": lines of the function, "meta": {key: value}}"""
    lines = text.split("\n")
    res: dict[str, dict] = {}
    cur = last = None
    for ln in lines:
        if last is not None and "; codeLenInByte = " in ln:       # (the comment block behind the function's end)
            res[last]["meta"].setdefault("code_bytes", ln.split("=")[1].split()[0])
        m = LABEL.match(ln)
        if m and not m.group(1).startswith((".L", "BB")) and cur is None and m.group(1).startswith("_Z"):
            cur = last = m.group(1)
            res[cur] = {"body": [], "meta": {}}
            continue
        if cur is not None:
            if ln.startswith(".Lfunc_end") or ln.strip().startswith(".section") or ln.strip().startswith(".amdhsa_kernel"):
                cur = None
                continue
            res[cur]["body"].append(ln)
    # the kernel descriptors' and the metadata's numbers
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        if m.group(1) in res:
            for k, v in re.findall(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset)\s+(\S+)", m.group(2)):
                res[m.group(1)]["meta"][k] = v
    for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if nm and nm.group(1) in res:
            for k in ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size"):
                v = re.search(r"\." + k + r":\s+(\d+)", blk)
                if v:
                    res[nm.group(1)]["meta"][k] = v.group(1)
    return res


def segments(body: list[str]) -> list[Counter]:
    segs, cur = [], Counter()
    for ln in body:
        m = INSTR.match(ln)
        if not m or ln.lstrip().startswith((".", ";")):
            continue
        op = m.group(1)
        if op == "s_barrier":
            cur["barrier"] += 1
            segs.append(cur)
            cur = Counter()
            continue
        cur[classify(op)] += 1
        if op.startswith(("v_writelane", "v_readlane")):
            cur["lane"] += 1
        if op.startswith("v_rcp_iflag"):
            cur["idiv"] += 1
    segs.append(cur)
    return segs


def report(name: str, k: dict, top: int) -> str:
    out = [name]
    meta = k["meta"]
    out.append("  " + "  ".join(f"{key} {meta[key]}" for key in ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count",
                                                                 "private_segment_fixed_size", "code_bytes") if key in meta))
    segs = segments(k["body"])
    tot = Counter()
    for s in segs:
        tot.update(s)
    n_all = sum(tot[c] for c in CLASSES) + tot["barrier"]
    out.append(f"  instructions {n_all}  barriers {tot['barrier']}  v_writelane/v_readlane {tot['lane']}  "
               f"integer divisions (v_rcp_iflag) {tot['idiv']}")
    out.append("  " + "  ".join(f"{c} {tot[c]}" for c in CLASSES))
    hdr = f"  {'seg':>4} {'all':>6} " + " ".join(f"{c:>6}" for c in CLASSES)
    out.append(hdr)
    rows = []
    for i, s in enumerate(segs):
        n = sum(s[c] for c in CLASSES)
        rows.append((i, n, s))
    show = rows if top <= 0 else sorted(sorted(rows, key=lambda r: -r[1])[:top])
    for i, n, s in show:
        out.append(f"  {i:>4} {n:>6} " + " ".join(f"{s[c]:>6}" for c in CLASSES))
    with_m = [n for _, n, s in rows if s["mfma"]]
    without = [n for _, n, s in rows if not s["mfma"]]
    scal = lambda s: s["sload"] + s["wait"] + s["br"] + s["salu"]
    out.append(f"  segments with MFMAs {len(with_m)}: {sum(with_m)} instructions, scalar share "
               f"{sum(scal(s) for _, _, s in rows if s['mfma'])}")
    out.append(f"  segments without    {len(without)}: {sum(without)} instructions, scalar share "
               f"{sum(scal(s) for _, _, s in rows if not s['mfma'])}")
    return "\n".join(out)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="device assembly of fused_ddpg.hip (default: compile it)")
    ap.add_argument("--filter", default="k_ddpg_chain", help="substring of the demangled kernel name")
    ap.add_argument("--top", type=int, default=0, help="only the N longest segments (0: all)")
    a = ap.parse_args()
    text = Path(a.asm).read_text() if a.asm else device_asm()
    ks = kernels(text)
    names = demangle(list(ks))
    for mangled in ks:
        nice = names.get(mangled, mangled)
        if a.filter in nice:
            print(report(nice.split("(")[0], ks[mangled], a.top))
            print()


if __name__ == "__main__":
    main()
