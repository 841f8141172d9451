"""The generated pairing constants are current, and equal the big-integer restatement's."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_pairing_consts_header_is_current(tmp_path, monkeypatch):
    sys.path.insert(0, str(ROOT / "tools"))
    try:
        import gen_pairing_consts
    finally:
        sys.path.pop(0)
    out = tmp_path / "pairing_consts.hpp"
    monkeypatch.setattr(gen_pairing_consts, "OUT", out)
    monkeypatch.setattr(gen_pairing_consts, "ROOT", tmp_path)
    gen_pairing_consts.main()
    assert out.read_text() == (ROOT / "dusk-plonk_amd" / "csrc" / "pairing_consts.hpp").read_text()


def test_generator_constants_agree_with_the_reference_pairing():
    sys.path.insert(0, str(ROOT / "tools"))
    try:
        import gen_pairing_consts as G
    finally:
        sys.path.pop(0)
    import pairing_ref as R
    assert G.P == R.p and G.X_ABS == R.X_ABS and G.G2_GEN == R.G2_GEN and G.XI == R.XI
