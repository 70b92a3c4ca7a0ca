"""Per-XCD dealing of an ordered batch's tickets (csrc/device_tickets.h) on the SIMT-emulated library: the product's own beam-kernel
source executed on the CPU.  Ordered batches of nq not a multiple of 8 * C, dealt in chunks of 2 and 4 (one-wave form at 96 dims, team
form at 768), return the oracle's labels, distance bits, counts and evaluation / hop counts and equal the global ticket's outputs — with
the emulator's stand-in XCD ids (blockIdx.x % 8) and with every wave on one counter (PGEMB_EMU_XCD_ID), where stealing carries the batch."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_xcd_tickets_case.py")


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu.build()


@pytest.mark.parametrize("xcd", [None, "0", "5"])
def test_dealt_batches_equal_the_oracle(emu_lib, xcd):
    env = dict(os.environ)
    env.pop("PGEMB_EMU_XCD_ID", None)
    if xcd is not None:
        env["PGEMB_EMU_XCD_ID"] = xcd
    r = subprocess.run([sys.executable, RUN, emu_lib], capture_output=True, text=True, timeout=1500, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res) == 4
    bad = [x for x in res if x["wrong"] or not x["same_as_global"] or not x["ordered"] or x["dealt"] != x["chunk"]]
    assert not bad, bad
    assert any("true" in x["kernel"].split(",")[3] for x in res), [x["kernel"] for x in res]   # team form
