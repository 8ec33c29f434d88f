"""What the recorders of tests/golden/*_forms.json share (make_golden_gemm_forms.py, make_golden_attention_forms.py).

A recorder runs the dispatch code of a git revision on the host, with hipLaunchKernelGGL re-defined to print instead of launching:

  extract          `git show REVISION:...` of csrc files and the C header into a scratch directory laid out like the repository
  build_host_only  hipcc --cuda-host-only of those sources behind a forced prelude, linked with a driver and empty device code bundles
  kernel_names     address -> mangled name of the recorder's kernel symbols (what the prelude printed -> which instance it was)
  template_args    mangled instance name -> (kernel, template arguments as integers)
"""
from __future__ import annotations

import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "boxdreamer_amd/csrc"


def sh(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)}\n{r.stderr}")
    return r.stdout


def extract(rev: str, tmp: str, files, edit=None) -> str:
    """Writes REVISION's csrc `files` (each passed through edit(name, text) if given) and its C header under tmp; returns tmp's csrc."""
    csrc = os.path.join(tmp, *CSRC.split("/"))                  # the repository's layout: bd_common.h includes ../../include/
    os.makedirs(csrc)
    os.makedirs(os.path.join(tmp, "include"))
    for f in files:
        src = sh(["git", "-C", ROOT, "show", f"{rev}:{CSRC}/{f}"])
        open(os.path.join(csrc, f), "w").write(edit(f, src) if edit else src)
    open(os.path.join(tmp, "include", "boxdreamer_hip.h"), "w").write(sh(["git", "-C", ROOT, "show", f"{rev}:include/boxdreamer_hip.h"]))
    return csrc


def build_host_only(tmp: str, sources, prelude: str, driver: str) -> str:
    """Compiles `sources` and the driver text for the host only, `prelude` forced in front of each; returns the executable."""
    open(os.path.join(tmp, "prelude.h"), "w").write(prelude)
    open(os.path.join(tmp, "driver.cpp"), "w").write(driver)
    hipcc = os.environ.get("HIPCC", "hipcc")
    exe = os.path.join(tmp, "recorder")
    objs = []
    for src in (*sources, os.path.join(tmp, "driver.cpp")):
        objs.append(src + ".o")
        sh([hipcc, "--cuda-host-only", "-O1", "-std=c++17", "-I", os.path.join(tmp, "include"), "-include", os.path.join(tmp, "prelude.h"),
            "-x", "hip", "-c", src, "-o", objs[-1]])
    # a host-only object still refers to the device code bundle it would register: give each an empty one (nothing is ever launched)
    fatbins = sorted({ln.split()[-1] for o in objs for ln in sh(["nm", "-u", o]).splitlines() if "__hip_fatbin_" in ln})
    open(os.path.join(tmp, "fatbins.c"), "w").write("".join(f"const char {n}[64] = {{0}};\n" for n in fatbins))
    sh([hipcc, "-no-pie", *objs, os.path.join(tmp, "fatbins.c"), "-o", exe])
    return exe


def kernel_names(exe: str, marker: str) -> dict:
    """address (hex, as a recorder prints it) -> mangled name of every symbol of the recorder (not position-independent) that has `marker`."""
    names = {}
    for line in sh(["nm", exe]).splitlines():
        addr, name = line.partition(" ")[0], line.split(" ")[-1]
        if marker in name and addr:
            names.setdefault(format(int(addr, 16), "x"), name)
    return names


# Itanium mangling of the template arguments the kernels take: __bf16, _Float16, fp8e4 (global), int, bool
ARG = r"DF16b|DF16_|5fp8e4|Lin?\d+E|Lb[01]E"
TOKEN = re.compile(r"(DF16b)|(DF16_)|(5fp8e4)|Li(n?\d+)E|Lb([01])E")


def template_args(mangled: str, kernel: str):
    """`_ZN12_GLOBAL__N_1..14gemm_kernel_pcIDF16bLi1ELi64E...EEv12bd_gemm_args` with kernel = a regex of kernel names ->
    ("gemm_kernel_pc", [0, 1, 64, ...]): types as 0 __bf16, 1 _Float16, 2 fp8e4, bools as 0 / 1."""
    m = re.search(r"\d+(" + kernel + r")I((?:" + ARG + r")+)E", mangled)
    if not m:
        raise SystemExit(f"cannot parse kernel name: {mangled}")
    key = []
    for t in TOKEN.finditer(m.group(2)):
        bf, f16, f8, i, b = t.groups()
        key.append(0 if bf else 1 if f16 else 2 if f8 else int(b) if b is not None else int(i.replace("n", "-")))
    return m.group(1), key
