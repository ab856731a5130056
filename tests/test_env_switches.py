"""Every FMX_* environment variable the package and the library read is listed in
INTEGRATION.md's "Environment switches" table, and nothing else is: a new switch needs a
line there.  The A/B arms that used to sit behind runtime switches stay out (an experiment
is a library of its own, ``make var`` + FMX_LIB)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "factormodeling_amd")

REMOVED = {
    "FMX_GRAM_MASK_MFMA", "FMX_GRAM_SINGLE_BUFFER", "FMX_GRAM_OPT", "FMX_GRAM_CNT", "FMX_GRAM_XCD", "FMX_GRAM_WOPT",
    "FMX_GRAM_ZC", "FMX_GRAM_GLDS", "FMX_GRAM_ZC_NT", "FMX_GRAM_MATERIALIZE", "FMX_TS_SET_SPLIT", "FMX_TS_SET_NT",
    "FMX_TS_CORR_V1", "FMX_CORR_FEAT_PF", "FMX_CS_MOMENT_LDS", "FMX_CS_NT", "FMX_GROUP_SORTED", "FMX_ZN_T64",
    "FMX_BR_NT", "FMX_FA_NT", "FMX_RANK_PASS_MAX_A",
}


def _read(path):
    with open(path, encoding="utf-8") as fh:
        return fh.read()


def native_switches():
    names = set()
    for ext in ("hip", "hpp", "cpp"):
        for path in glob.glob(os.path.join(PKG, "csrc", f"*.{ext}")):
            names.update(re.findall(r'getenv\(\s*"(FMX_[A-Z0-9_]+)"\s*\)', _read(path)))
    return names


def python_switches():
    names = set()
    for path in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True):
        names.update(re.findall(r'os\.environ(?:\.get\(|\[)\s*"(FMX_[A-Z0-9_]+)"', _read(path)))
    return names


def documented_switches():
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    m = re.search(r"^## [^\n]*Environment switches\n(.*?)(?=^## |\Z)", text, re.S | re.M)
    assert m, "INTEGRATION.md has no 'Environment switches' section"
    return set(re.findall(r"^\|\s*`(FMX_[A-Z0-9_]+)`\s*\|", m.group(1), re.M))


def test_switch_table_matches_the_code():
    assert len(REMOVED) == 21
    native, py = native_switches(), python_switches()
    assert native and py                    # the scans found the sources
    read = native | py
    assert read == documented_switches()
    assert not read & REMOVED
