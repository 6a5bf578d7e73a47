"""CPU-side check (-m "not gpu") that the list of environment switches in INTEGRATION.md is complete: every M2M_* variable
the Python package reads (the table in m2_mixer_amd/config.py), every one the library reads (m2m_env_int in csrc), and that
the package reads the environment nowhere but through that table."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "m2_mixer_amd")
#: the files that may touch os.environ: the table and its readers, the library path (read before config can be imported),
#: torchrun's RANK / WORLD_SIZE / MASTER_* contract
ENV_FILES = {"config.py", "_lib.py", "parallel.py"}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def test_every_switch_is_documented_and_read_in_one_place():
    from m2_mixer_amd import config
    doc = set(re.findall(r"M2M_[A-Z0-9_]+", _read(os.path.join(ROOT, "INTEGRATION.md"))))
    table = set(config.SWITCHES)
    assert table and all(n.startswith("M2M_") for n in table)
    assert not table - doc, f"switches of config.SWITCHES missing from INTEGRATION.md: {sorted(table - doc)}"

    csrc = "".join(_read(p) for p in sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h"))))
    calls = re.findall(r"m2m_env_int\(\s*([^,)]*)", csrc)
    names = {m.group(1) for m in (re.fullmatch(r'"(M2M_[A-Z0-9_]+)"', c.strip()) for c in calls) if m}
    # every call but the function's own definition (`const char* name`) passes a literal: nothing escapes the search
    assert len(names) >= 10 and sum(1 for c in calls if not c.strip().startswith('"')) == 1, calls
    assert not names - doc, f"switches the library reads (m2m_env_int) missing from INTEGRATION.md: {sorted(names - doc)}"

    py = [p for p in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True) if os.path.basename(p) not in ENV_FILES]
    assert len(py) >= 8
    leaks = [os.path.relpath(p, ROOT) for p in py if "os.environ" in _read(p)]
    assert not leaks, f"os.environ outside config.py / _lib.py / parallel.py: {leaks}"


def test_switch_readers(monkeypatch):
    """The readers look at the environment when called; default-on switches are off only for "0", default-off ones on only for "1"."""
    from m2_mixer_amd import config
    for name in ("M2M_CONCURRENT", "M2M_EMBED_FOLD", "M2M_FUSED_UPDATE", "M2M_MIMIC_STREAMS"):
        monkeypatch.delenv(name, raising=False)
    assert config.switch_on("M2M_CONCURRENT") and not config.switch_on("M2M_EMBED_FOLD")
    assert config.switch("M2M_FUSED_UPDATE") is None and config.switch("M2M_MIMIC_STREAMS", "both") == "both"
    for value, on_default, off_default in (("0", False, False), ("1", True, True), ("2", True, False), ("", True, False)):
        monkeypatch.setenv("M2M_CONCURRENT", value)
        monkeypatch.setenv("M2M_EMBED_FOLD", value)
        assert config.switch_on("M2M_CONCURRENT") is on_default and config.switch_on("M2M_EMBED_FOLD") is off_default
    monkeypatch.setenv("M2M_MIMIC_STREAMS", "fwd")
    assert config.switch("M2M_MIMIC_STREAMS", "both") == "fwd"
