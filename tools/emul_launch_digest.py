#!/usr/bin/env python3
"""Which kernel instantiation, grid, block and dynamic LDS every host launcher picks, pinned through the CPU emulator.

Runs each tests/test_emul_*.py with pytest in a child process under CFD_EMUL_LAUNCH_LOG (tests/emul/include/hip/hip_runtime.h: one line
per launch) and writes one JSON: per file the number of launches, the SHA-256 of the log and the sorted distinct instantiations.

    python tools/emul_launch_digest.py -o profiles/emul_launches.json [--keep-logs DIR] [test_emul_x.py ...]
    python tools/emul_launch_digest.py --compare OTHER.json [-i THIS.json] [--keep-logs DIR --other-logs DIR]

--compare prints the first differing file and exits with status 1 (0: identical).  The JSON holds digests, not the logs: the first
differing RECORD is printed only when both runs kept their raw logs and both directories are given (--keep-logs DIR --other-logs DIR);
without them it prints the instantiations that only one side launched.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def run_file(test: Path, logdir: Path) -> dict:
    """One log per process ("%p": some files run their cases in parallel children), joined in the order of the logs' own SHA-256 -- the
    sequence inside a process is kept, and the whole does not depend on process ids or on which child finished first."""
    stem = test.stem
    for old in logdir.glob(stem + ".*log"):
        old.unlink()
    env = dict(os.environ, CFD_EMUL_LAUNCH_LOG=str(logdir / (stem + ".%p.plog")))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", str(test)], cwd=REPO, env=env, capture_output=True,
                       text=True)
    if r.returncode != 0:
        print(r.stdout[-3000:], file=sys.stderr)
    parts = sorted((f.read_bytes() for f in logdir.glob(stem + ".*.plog")), key=lambda b: hashlib.sha256(b).hexdigest())
    for f in logdir.glob(stem + ".*.plog"):
        f.unlink()
    data = b"".join(parts)
    (logdir / (stem + ".log")).write_bytes(data)
    lines = data.decode().splitlines()
    return {
        "pytest_exit": r.returncode,
        "launches": len(lines),
        "sha256": hashlib.sha256(data).hexdigest(),
        "instantiations": sorted({ln.split(" grid ")[0] for ln in lines}),
    }


def first_difference(name: str, a: dict, b: dict, logs, other_logs) -> str:
    msg = [f"{name}: launches {a['launches']} vs {b['launches']}, sha256 {a['sha256'][:12]} vs {b['sha256'][:12]}"]
    stem = Path(name).stem + ".log"
    la, lb = Path(logs or "", stem), Path(other_logs or "", stem)
    if logs and other_logs and la.is_file() and lb.is_file():
        xa, xb = la.read_text().splitlines(), lb.read_text().splitlines()
        for i in range(max(len(xa), len(xb))):
            ra, rb = (xa[i] if i < len(xa) else "<end>"), (xb[i] if i < len(xb) else "<end>")
            if ra != rb:
                msg += [f"  record {i}:", f"    this:  {ra}", f"    other: {rb}"]
                break
    else:  # no raw logs kept: the instantiations that only one side launched
        sa, sb = set(a["instantiations"]), set(b["instantiations"])
        msg += [f"  only this:  {s}" for s in sorted(sa - sb)[:5]] + [f"  only other: {s}" for s in sorted(sb - sa)[:5]]
    return "\n".join(msg)


def compare(this: dict, other: dict, logs=None, other_logs=None) -> int:
    for name in sorted(set(this) | set(other)):
        a, b = this.get(name), other.get(name)
        if a is None or b is None:
            print(f"{name}: only in {'other' if a is None else 'this'}")
            return 1
        if (a["launches"], a["sha256"], a["instantiations"]) != (b["launches"], b["sha256"], b["instantiations"]):
            print(first_difference(name, a, b, logs, other_logs))
            return 1
    print(f"identical: {len(this)} files, {sum(v['launches'] for v in this.values())} launches")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tests", nargs="*", help="test files (default: every tests/test_emul_*.py)")
    ap.add_argument("-o", "--output", help="where the JSON goes (default: stdout)")
    ap.add_argument("-i", "--input", help="with --compare: a JSON made earlier instead of a fresh run")
    ap.add_argument("--keep-logs", metavar="DIR", help="keep the raw logs there (with -i: where that run kept them)")
    ap.add_argument("--other-logs", metavar="DIR", help="with --compare: the raw logs of OTHER.json's run; needed, with --keep-logs, to name the first differing record")
    ap.add_argument("--compare", metavar="OTHER.json")
    args = ap.parse_args()

    if args.input:
        result = json.loads(Path(args.input).read_text())
    else:
        tests = [Path(t).resolve() for t in args.tests] or sorted((REPO / "tests").glob("test_emul_*.py"))
        with tempfile.TemporaryDirectory() as tmp:
            logdir = Path(args.keep_logs).resolve() if args.keep_logs else Path(tmp)
            logdir.mkdir(parents=True, exist_ok=True)
            result = {}
            for t in tests:
                result[t.name] = run_file(t, logdir)
                print(f"{t.name}: {result[t.name]['launches']} launches, pytest exit {result[t.name]['pytest_exit']}", file=sys.stderr)
        text = json.dumps(result, indent=1, sort_keys=True) + "\n"
        if args.output:
            Path(args.output).write_text(text)
        elif not args.compare:
            sys.stdout.write(text)
    if args.compare:
        return compare(result, json.loads(Path(args.compare).read_text()), args.keep_logs, args.other_logs)
    return 0 if all(v["pytest_exit"] == 0 for v in result.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
