"""The compiler's own resource remarks (-Rpass-analysis=kernel-resource-usage) of one translation unit of lurk_beta_amd/csrc, for the
tests that hold kernels to register and scratch budgets."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lurk_beta_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-unused-variable"]


def usage(src, out_dir):
    """{mangled kernel name: {"vgprs", "agprs", "scratch" (bytes per lane)}} of csrc/<src>, compiled for gfx950 into out_dir."""
    r = subprocess.run(["hipcc", *FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(out_dir, src + ".o")], cwd=CSRC,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]
    out, name = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, ln)
            if m and name:
                out[name][key] = int(m.group(1))
    return out
