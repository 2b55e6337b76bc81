"""Build the product HIP sources against the CPU SIMT emulator (tests/emul/include) into
tests/emul/_build/libcfd_emul.so.  TEST INFRASTRUCTURE ONLY -- never used by the product path.

build(sanitize=True) compiles the same sources with -fsanitize=alignment (host code, CPU only) into
tests/emul/_build/san/libcfd_emul_san.so, linked against clang's shared UBSan runtime by rpath: a load or store through a
pointer type whose alignment the address does not have prints "file:line: runtime error: ... misaligned address" on stderr."""
from __future__ import annotations

import hashlib
import os
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
CSRC = REPO / "cfdbench_amd" / "csrc"
OUT = HERE / "_build"
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def sources():
    return sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.cpp"))) + [HERE / "fiber_switch.cpp"]


def _ubsan_runtime() -> Path:
    rdir = Path(subprocess.run([CLANG, "-print-resource-dir"], check=True, capture_output=True, text=True).stdout.strip())
    hits = sorted(rdir.glob("lib/*/libclang_rt.ubsan_standalone-x86_64.so")) + sorted(rdir.glob("lib/*/libclang_rt.ubsan_standalone.so"))
    if not hits:
        raise FileNotFoundError(f"no shared UBSan runtime under {rdir}")
    return hits[0]


def build(force: bool = False, sanitize: bool = False) -> Path:
    out_dir = OUT / "san" if sanitize else OUT
    out_dir.mkdir(parents=True, exist_ok=True)
    lib = out_dir / ("libcfd_emul_san.so" if sanitize else "libcfd_emul.so")
    # (-O1 -g1: the reports carry file:line, and the build stays near the default one's time)
    opt = ["-O1", "-g1", "-fsanitize=alignment"] if sanitize else ["-O2"]
    h = hashlib.sha1()
    for f in sources() + sorted(CSRC.glob("*.h")) + sorted((HERE / "include").rglob("*.h")) + [REPO / "include" / "cfdbench_amd.h"]:
        h.update(f.read_bytes())
    stamp = out_dir / "stamp"
    if lib.exists() and stamp.exists() and stamp.read_text() == h.hexdigest() and not force:
        return lib
    hdr = hashlib.sha1()
    for f in sorted(CSRC.glob("*.h")) + sorted((HERE / "include").rglob("*.h")) + [REPO / "include" / "cfdbench_amd.h"]:
        hdr.update(f.read_bytes())

    def compile_one(src: Path) -> str:
        obj = out_dir / (src.name + ".o")
        ostamp = out_dir / (src.name + ".stamp")  # per-object stamp: one edited kernel file recompiles alone
        odig = hashlib.sha1(hdr.digest() + src.read_bytes()).hexdigest()
        if obj.exists() and ostamp.exists() and ostamp.read_text() == odig and not force:
            return str(obj)
        cmd = [CLANG, "-x", "c++", "-std=c++20", *opt, "-fPIC", "-pthread", "-Wno-unused-value",
               f"-I{HERE / 'include'}", f"-I{CSRC}", f"-I{REPO / 'include'}", "-DCFD_CONV6_GRID=2", "-DCFD_CONVT6_NT4_MIN_WGS=2", "-DCFD_CONV1_NT4_MIN_WGS=2", "-c", str(src), "-o",
               str(obj)]
        subprocess.run(cmd, check=True)
        ostamp.write_text(odig)
        return str(obj)

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:  # one translation unit per core (was serial: 4 minutes)
        objs = list(ex.map(compile_one, sources()))
    link = []
    if sanitize:
        rt = _ubsan_runtime()
        link = [str(rt), f"-Wl,-rpath,{rt.parent}"]
    subprocess.run([CLANG, "-shared", "-pthread", "-o", str(lib)] + objs + link, check=True)
    stamp.write_text(h.hexdigest())
    return lib


if __name__ == "__main__":
    import sys
    print(build(force=True, sanitize="--sanitize" in sys.argv[1:]))
