"""Layout of the streaming kernel's LDS control block (csrc/stream_dev.h, struct Ctl) that its
wide counter reads rely on: each direction's converter / gradient counters form one aligned
16-byte group (one LDS read per poll), conv / help are the first 4 * kMaxW words (the kernel's
initial fill addresses them by word index), and the chain's own words (chain, sread: single-word
stores and reads) lie outside those groups. CPU only: a tiny host program compiled from the
header."""
import json
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ssnt-tts-rust_amd" / "csrc"

PROG = r"""
#include <cstddef>
#include <cstdio>
#include "stream_dev.h"
int main() {
  using namespace ssnt;
  std::printf("{\"sizeof\": %zu, \"alignof\": %zu, \"kCtlBytes\": %zu, \"kMaxW\": %d, "
              "\"conv0\": %zu, \"conv1\": %zu, \"help0\": %zu, \"help1\": %zu, "
              "\"chain\": %zu, \"sread\": %zu}\n",
              sizeof(Ctl), alignof(Ctl), (size_t)kCtlBytes, kMaxW,
              offsetof(Ctl, conv[0]), offsetof(Ctl, conv[1]), offsetof(Ctl, help[0]), offsetof(Ctl, help[1]),
              offsetof(Ctl, chain), offsetof(Ctl, sread));
  return 0;
}
"""


def _hipcc():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    return shutil.which("hipcc") or str(Path(rocm) / "bin" / "hipcc")


@pytest.mark.parametrize("defs", [[], ["-DSSNT_DIAG"]], ids=["product", "diag"])
def test_ctl_layout(tmp_path, defs):
    src = tmp_path / "ctl_layout.hip"
    src.write_text(PROG)
    exe = tmp_path / "ctl_layout"
    subprocess.run([_hipcc(), "--cuda-host-only", "-std=c++17", "-Wno-invalid-offsetof", "-I", str(ROOT / "include"),
                    "-I", str(CSRC), *defs, str(src), "-o", str(exe)], check=True)
    L = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert L["kMaxW"] == 4 and L["sizeof"] <= L["kCtlBytes"] and L["alignof"] >= 16
    # the initial fill: conv = words [0, 2 kMaxW), help = words [2 kMaxW, 4 kMaxW)
    assert (L["conv0"], L["conv1"], L["help0"], L["help1"]) == (0, 16, 32, 48)
    for k in ("conv0", "conv1", "help0", "help1"):
        assert L[k] % 16 == 0, k  # one 16-byte read per direction
    assert L["chain"] >= 64 and L["sread"] >= 64 and L["chain"] % 4 == 0 and L["sread"] % 4 == 0
