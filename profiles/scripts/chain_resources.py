"""Register / scratch / occupancy table of every chain-step kernel instantiation, and the comparison of two such tables.

  python profiles/scripts/chain_resources.py table [--csrc DIR] [--jobs N] [--units PATTERN ...] OUT.json
      compiles the device side of every chain_fused_i*.hip, chain_wide_i*.hip and chain_sum_i*.hip of DIR (default: this
      tree's tt_sketch_amd/csrc) for gfx950 with -Rpass-analysis=kernel-resource-usage and records, per kernel:
      SGPRs, VGPRs, AGPRs, ScratchSize, Occupancy, SGPR and VGPR spills, LDS size.  No GPU needed.
      --units names other units by glob patterns, e.g. hadamard_apply.hip hadamard_close.hip op_apply.hip.
  python profiles/scripts/chain_resources.py compare PARENT.json NEW.json
      the rule a restructuring of these kernels has to keep: per kernel equal ScratchSize and spill counts, occupancy not
      lower; lists every kernel whose VGPR count moved by more than 8.  Exit status 1 if the rule is broken.

Build the parent's table from a checkout of the parent commit (git worktree add DIR <commit>; --csrc DIR/tt_sketch_amd/csrc).
"""
import argparse
import concurrent.futures
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIELDS = {
    "TotalSGPRs": "sgpr", "VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch",
    "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill",
    "LDS Size [bytes/block]": "lds",
}


def hipcc():
    return "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"


def unit_table(src, csrc):
    cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-c", src, "-o", os.devnull]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr[-2000:]}")
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+([^:]+):\s+(\S+)", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault(demangle(val), {})
        elif cur is not None and key in FIELDS:
            cur[FIELDS[key]] = int(val)
    return out


_demangled = {}


def demangle(name):
    if name not in _demangled:
        try:
            _demangled[name] = subprocess.run(["c++filt", name], stdout=subprocess.PIPE, text=True, check=True).stdout.strip()
        except (OSError, subprocess.CalledProcessError):
            _demangled[name] = name                # no c++filt: the mangled name serves as the key just as well
    return _demangled[name]


CHAIN_UNITS = ("chain_fused_i*.hip", "chain_wide_i*.hip", "chain_sum_i*.hip")


def table(csrc, jobs, out, only=None, units=CHAIN_UNITS):
    srcs = sorted(s for pat in units for s in glob.glob(os.path.join(csrc, pat)))
    if only:
        srcs = [s for s in srcs if re.search(only, os.path.basename(s))]
    if not srcs:
        raise SystemExit(f"no unit matches {' '.join(units)} under {csrc}")
    kernels = {}
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        for src, t in zip(srcs, ex.map(lambda s: unit_table(s, csrc), srcs)):
            print(f"{os.path.basename(src)}: {len(t)} kernels", flush=True)
            kernels.update(t)
    with open(out, "w") as f:
        json.dump(kernels, f, indent=0, sort_keys=True)
    print(f"{len(kernels)} kernels -> {out}")


def compare(parent, new):
    with open(parent) as f:
        P = json.load(f)
    with open(new) as f:
        N = json.load(f)
    bad, moved = [], []
    if set(N) - set(P):
        bad.append(f"kernels the parent does not have: {sorted(set(N) - set(P))[:3]}")
    if set(P) - set(N):                      # a table made with --only holds some of the units
        print(f"note: {len(set(P) - set(N))} kernels of the parent's table are not in the new one")
    for k in sorted(set(P) & set(N)):
        p, n = P[k], N[k]
        for fld in ("scratch", "sgpr_spill", "vgpr_spill"):
            if p[fld] != n[fld]:
                bad.append(f"{k}: {fld} {p[fld]} -> {n[fld]}")
        if n["occupancy"] < p["occupancy"]:
            bad.append(f"{k}: occupancy {p['occupancy']} -> {n['occupancy']}")
        if abs(n["vgpr"] - p["vgpr"]) > 8:
            moved.append(f"{k}: VGPRs {p['vgpr']} -> {n['vgpr']}")
    print(f"{len(set(P) & set(N))} kernels compared")
    print(f"VGPR count moved by more than 8: {len(moved)}")
    for m in moved:
        print("  " + m)
    print(f"scratch / spill / occupancy rule broken: {len(bad)}")
    for b in bad:
        print("  " + b)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("table")
    t.add_argument("--csrc", default=os.path.join(ROOT, "tt_sketch_amd", "csrc"))
    t.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    t.add_argument("--only", default=None, help="regular expression: only the units whose file name matches")
    t.add_argument("--units", nargs="+", default=CHAIN_UNITS, metavar="PATTERN", help="glob patterns of the units under --csrc")
    t.add_argument("out")
    c = sub.add_parser("compare")
    c.add_argument("parent")
    c.add_argument("new")
    a = ap.parse_args()
    if a.cmd == "table":
        table(a.csrc, a.jobs, a.out, a.only, a.units)
    else:
        sys.exit(compare(a.parent, a.new))


if __name__ == "__main__":
    main()
