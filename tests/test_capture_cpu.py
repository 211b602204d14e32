"""CPU checks around output capture: the guest program `outs`
the GPU tests rest on assembles and its golden run on the oracle equals the
Python model; the re-validation harness's stdout comparison on hand-made
records; the host arithmetic of fi_run_sites_capture (argument check, row
pitch, chunk sizing, staging copy: fi_capture.h) in a stand-alone host program
under AddressSanitizer and UBSan."""
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

M64 = (1 << 64) - 1
OUTS_NINST, OUTS_EXIT = 14146, 7


def outs_source() -> str:
    """Writes 8 bytes to stdout in each of 24 rounds of 64 xorshift steps, and
    "err!\\n" to stderr in every fourth: output all along the run, a counted
    inner loop, and a round counter (s1) whose flip makes a long run that
    keeps printing."""
    return """    .text
_start:
    la    s2, buf
    la    s3, msg
    li    s0, 0x1234567
    li    s1, 24
    li    s5, 0
round:
    li    t0, 64
inner:
    slli  t1, s0, 13
    xor   s0, s0, t1
    srli  t1, s0, 7
    xor   s0, s0, t1
    slli  t1, s0, 17
    xor   s0, s0, t1
    add   s0, s0, s5
    addi  t0, t0, -1
    bnez  t0, inner
    sd    s0, 0(s2)
    li    a0, 1
    mv    a1, s2
    li    a2, 8
    li    a7, 64
    ecall
    andi  t1, s5, 3
    li    t2, 3
    bne   t1, t2, skip
    li    a0, 2
    mv    a1, s3
    li    a2, 5
    li    a7, 64
    ecall
skip:
    addi  s5, s5, 1
    addi  s1, s1, -1
    bnez  s1, round
    li    a0, 7
    li    a7, 93
    ecall
    .data
msg:
    .byte 101, 114, 114, 33, 10
    .bss
    .balign 8
buf:
    .zero 8
"""


OUTS_MSG = b"err!\n"


def outs_model(msg: bytes = OUTS_MSG):
    """-> (stdout, stderr) of the fault-free run."""
    h, out, err = 0x1234567, b"", b""
    for r in range(24):
        for _ in range(64):
            h ^= (h << 13) & M64
            h ^= h >> 7
            h ^= (h << 17) & M64
            h = (h + r) & M64
        out += h.to_bytes(8, "little")
        if r & 3 == 3:
            err += msg
    return out, err


def outs_elf() -> bytes:
    from tools.rvasm.rvasm import assemble
    return assemble(outs_source())


def test_outs_program_on_oracle(oracle_mod):
    o = oracle_mod.Oracle(outs_elf(), "outs")
    g = o.run_golden()
    out, err = outs_model()
    assert (len(out), len(err)) == (192, 30)
    assert (g.ninst, g.exit_code) == (OUTS_NINST, OUTS_EXIT)
    assert o.golden_stdout() == out
    assert o.golden_stderr() == err
    # a fault-free serial run prints the same
    res, stdout = o.run_one(None)
    assert res["cls"] == 0 and stdout == out


def test_outs_campaign_on_oracle(oracle_mod):
    """The campaign the GPU tests run (seed 0x5EED0001, trials 0..1499,
    x1..x31 + pc + memory): what the oracle's serial runs print is varied
    enough to test capture with."""
    o = oracle_mod.Oracle(outs_elf(), "outs")
    o.run_golden()
    gold = outs_model()[0]
    sites = o.sample(0x5EED0001, 0, 1500, ((1 << 32) - 2) | (1 << 32) | (1 << 33))
    runs = [o.run_one(s) for s in sites]
    cls = np.bincount([int(r[0]["cls"]) for r in runs], minlength=6).tolist()
    assert cls == [1202, 112, 114, 72, 0, 0]
    sdc = [out for r, out in runs if r["cls"] == 1]
    assert sum(len(out) == len(gold) and out != gold for out in sdc) == 97
    assert max(len(out) for _, out in runs) == 392


def test_campaign_outputs_refuses_timing():
    """Checked before anything runs, so with no engine behind the object."""
    import pytest
    from shrewd_amd import FaultCampaign
    c = FaultCampaign.__new__(FaultCampaign)
    c.cpu_type = "timing"
    with pytest.raises(ValueError, match="timing"):
        c.outputs([1, 2])


def test_revalidate_stdout_check():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gem5_revalidate import stdout_check
    cap = 16
    row = np.zeros(cap, np.uint8)
    row[:5] = list(b"hello")
    assert stdout_check(b"hello", row, 5) is True
    assert stdout_check(b"hellp", row, 5) is False          # other bytes
    assert stdout_check(b"hell", row, 5) is False           # other length
    assert stdout_check(b"hello\0", row, 5) is False
    assert stdout_check(b"", np.zeros(cap, np.uint8), 0) is True
    full = np.frombuffer(b"0123456789abcdef", np.uint8)
    assert stdout_check(b"0123456789abcdef", full, cap) is True           # exactly the cap: compared
    assert stdout_check(b"0123456789abcdefgh", full, cap + 2) is None     # truncated at the cap: skipped
    assert stdout_check(b"something else", full, cap + 2) is None


def test_capture_host_arithmetic_sanitized(tmp_path):
    """tools/capture_host_check.cpp: fi_capture.h's functions, as the engine
    calls them, in a host program of its own under ASan and UBSan."""
    csrc = os.path.join(ROOT, "shrewd_amd", "csrc")
    exe = str(tmp_path / "capture_host_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                    os.path.join(ROOT, "tools", "capture_host_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "capture_host_check ok" in r.stdout
