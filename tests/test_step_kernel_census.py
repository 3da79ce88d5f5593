"""The step kernel family of c4_session.hip as hipcc builds it for gfx950: WHICH instantiations exist, and what each costs.

The host picks an instantiation by planes type and session mode (launch_step, c4_session_step_head_out, c4_session_start,
hold_launch_resume); a dispatch that quietly instantiates a kernel nobody launches, or loses one, changes this set.  The
registers and scratch of the hot kernels move with almost any edit of step_body (the step kernel): a change that
was meant to leave them alone fails here, and performance work updates the table on purpose.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from c4a0_amd.csrc import build as hip_build

# (kernel, template arguments after the planes type) -> VGPRs for f32 / bf16 planes (None: not built), scratch bytes per lane.
# c4_step_kernel <NOISE, CACHE, SEARCH, HOLD>, c4_step_gather_kernel <NOISE, CACHE>, c4_out_step_kernel <games per wavefront, SEARCH, HOLD>
CENSUS = {
    ("c4_step_kernel", (0, 0, 0, 0)): ((127, 128), 0),
    ("c4_step_kernel", (0, 1, 0, 0)): ((150, 151), 0),
    ("c4_step_kernel", (1, 0, 0, 0)): ((156, 157), 192),
    ("c4_step_kernel", (1, 1, 0, 0)): ((163, 164), 192),
    ("c4_step_kernel", (0, 0, 1, 0)): ((103, 103), 0),
    ("c4_step_kernel", (0, 0, 0, 1)): ((88, 90), 0),
    ("c4_step_gather_kernel", (0, 0)): ((127, 128), 0),
    ("c4_step_gather_kernel", (0, 1)): ((150, 151), 0),
    ("c4_step_gather_kernel", (1, 0)): ((156, 157), 192),
    ("c4_step_gather_kernel", (1, 1)): ((163, 164), 192),
    ("c4_out_step_kernel", (4, 0, 0)): ((151, 151), 0),
    ("c4_out_step_kernel", (8, 0, 0)): ((155, 155), 0),
    ("c4_out_step_kernel", (4, 1, 0)): ((None, 151), 0),
    ("c4_out_step_kernel", (8, 1, 0)): ((None, 153), 0),
    ("c4_out_step_kernel", (4, 0, 1)): ((None, 150), 0),
    ("c4_out_step_kernel", (8, 0, 1)): ((None, 152), 0),
    ("k_hold_resume", ()): ((145, 146), 0),
    ("c4_start_kernel", ()): ((34, 34), 0),
}
FAMILY = sorted({k for k, _ in CENSUS}, key=len, reverse=True)
# the Itanium name of an instantiation: <length><name>I<f = float | t = unsigned short><L b|j value E>...E
MANGLED = re.compile(r"\d+(" + "|".join(FAMILY) + r")I([ft])((?:L[bj]\d+E)*)E")


def test_step_kernel_census(tmp_path):
    """Exactly the 32 instantiations of the table, each with the table's VGPRs and scratch and without a spilled VGPR."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(hip_build.HERE, "c4_session.hip")
    flags = [f for f in hip_build.FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "session.s")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    built = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", r.stderr, re.S):
        name = MANGLED.search(m.group(1))
        if not name:
            continue
        key = (name.group(1), "f32" if name.group(2) == "f" else "bf16", tuple(int(v) for v in re.findall(r"L[bj](\d+)E", name.group(3))))
        assert key not in built, key
        built[key] = tuple(int(re.search(what + r": (\d+)", m.group(2)).group(1))
                           for what in (r" VGPRs", r"ScratchSize \[bytes/lane\]", r"VGPRs Spill"))
    want = {}
    for (kernel, args), (vgprs, scratch) in CENSUS.items():
        for planes, v in zip(("f32", "bf16"), vgprs):
            if v is not None:
                want[(kernel, planes, args)] = (v, scratch, 0)
    assert len(want) == 32
    assert sorted(built) == sorted(want), "missing: %s, extra: %s" % (sorted(set(want) - set(built)), sorted(set(built) - set(want)))
    wrong = {k: (built[k], want[k]) for k in want if built[k] != want[k]}
    assert not wrong, "(VGPRs, scratch bytes per lane, spilled VGPRs) built vs expected: %s" % wrong
