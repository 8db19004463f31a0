"""The C-ABI library (no GPU needed): it exists, loads, and exports exactly the symbols the
public header declares -- including the seven unmangled reference symbols the TF ops bind
(ssnt_tts_c/src/lib.rs:11,87,119,221,245,268,347). No compute calls here."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ssnt_tts_c.h"
AB_HEADER = ROOT / "include" / "ssnt_tts_c_ab.h"
LIB = ROOT / "ssnt-tts-rust_amd" / "lib" / "libssnt_tts_c.so"
AB_LIB = ROOT / "ssnt-tts-rust_amd" / "lib" / "ab" / "libssnt_tts_c_ab.so"

REFERENCE_SYMBOLS = [
    "ssnt_tts_beam_search_decode", "ssnt_extract_best_beam_branch",
    "ssnt_tts_v2_beam_search_decode", "ssnt_order_beam_branch", "ssnt_upsample_source_indexes",
    "tone_latent_beam_search_decode", "tone_latent_levenshtein_edit_distance",
]


def header_functions(header=HEADER):
    txt = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    txt = re.sub(r"#.*", "", txt)
    names = re.findall(r"\b([A-Za-z_]\w*)\s*\([^;{]*\)\s*;", txt)
    return sorted(set(n for n in names if n not in ("if", "while", "sizeof")))


def test_header_declares_reference_symbols():
    fns = header_functions()
    for s in REFERENCE_SYMBOLS:
        assert s in fns


def _exported(lib):
    assert lib.exists(), f"build the library first (make): {lib}"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True,
                         check=True).stdout
    return set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_library_exports_every_header_symbol():
    exported = _exported(LIB)
    missing = [f for f in header_functions() if f not in exported]
    assert not missing, f"declared but not exported: {missing}"


def test_product_exports_no_ab_knob():
    # the product's exported surface is the reference's 7 symbols plus the
    # extensions dispatch uses; the process-wide A/B knobs and diagnostics live only in the A/B
    # build (include/ssnt_tts_c_ab.h), so no caller can flip another thread's kernel
    exported = _exported(LIB)
    ab = header_functions(AB_HEADER)
    assert ab and not set(ab) & set(header_functions())
    leaked = sorted(f for f in exported if f in ab or "set_variant" in f or "diag" in f)
    assert not [f for f in exported if f.startswith("_Z")], "C++ internals exported (-fvisibility=hidden)"
    assert not leaked, f"A/B symbols in the product library: {leaked}"
    assert sorted(f for f in exported if f.startswith(("ssnt_", "tone_"))) == header_functions()


def test_ab_library_exports_both_headers():
    exported = _exported(AB_LIB)
    missing = [f for f in header_functions() + header_functions(AB_HEADER) if f not in exported]
    assert not missing, f"declared but not exported by the A/B build: {missing}"


def test_ctypes_binding_matches_header():
    from ssnt_tts_amd._lib import AB_SIGNATURES, SIGNATURES, load, load_ab
    assert sorted(SIGNATURES) == header_functions()
    assert sorted(AB_SIGNATURES) == header_functions(AB_HEADER)
    lib = load()  # dlopen only; no HIP call
    for name in SIGNATURES:
        assert getattr(lib, name) is not None
    ab = load_ab()
    for name in AB_SIGNATURES:
        assert getattr(ab, name) is not None


def test_reference_symbols_are_unmangled_c():
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True,
                         check=True).stdout
    for s in REFERENCE_SYMBOLS:
        assert re.search(rf"\bT {s}$", out, flags=re.M), s


def test_product_never_references_the_oracle():
    # the product path must not link, load or import anything under oracle/
    for p in (ROOT / "ssnt-tts-rust_amd").rglob("*"):
        if p.is_file() and p.suffix in (".hip", ".h", ".cpp", ".c"):
            code = re.sub(r"/\*.*?\*/|//[^\n]*", "", p.read_text(), flags=re.S)
            assert "oracle" not in code, p
        elif p.is_file() and p.suffix == ".py":
            code = "\n".join(l.split("#")[0] for l in p.read_text().splitlines())
            assert not re.search(r"^\s*(import|from)\s+oracle\b", code, flags=re.M), p
            assert "libssnt_oracle" not in code, p
    out = subprocess.run(["ldd", str(LIB)], capture_output=True, text=True).stdout
    assert "oracle" not in out


def test_mirror_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import ssnt_tts_amd as S
    with pytest.raises(RuntimeError):
        S.ssnt_fwd_bwd(torch.zeros(1, 2, 2, 2), torch.ones(1), torch.ones(1))


def test_segmented_workspace_query_covers_the_handoff_block():
    # host-only queries (no HIP call): the long-row kernel's workspace = the hand-off counter
    # block + the global hand-off rings + its rows (fwd_bwd_wide.hip wide_layout), each piece
    # padded to 256 B; the A/B build's hook for its workgroup split takes -1 / 0 / 1 only
    from ssnt_tts_amd._lib import load, load_ab
    lib = load()
    r256 = lambda x: (x + 255) & ~255  # noqa: E731
    for B, T, U in [(64, 2000, 400), (2, 1030, 1024), (3, 33, 300), (1, 1, 257)]:
        wide = r256(16 * B) + r256(B * 2 * (T + 64) * 8) + B * (T + 1) * U * 8
        stream = B * T * (U + 3) * 8
        assert lib.ssnt_fwd_bwd_workspace_size(B, T, U) == max(wide, stream), (B, T, U)
    ab = load_ab()
    for bad in (-2, 2, 3, 7):
        assert ab.ssnt_fwd_bwd_wide_split(bad) != 0
    for ok in (0, 1, -1):
        assert ab.ssnt_fwd_bwd_wide_split(ok) == 0
