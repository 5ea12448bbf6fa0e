"""The A/B harness (tools/tab_variants.py, tools/wide_variants.py) builds library variants as
source patches of csrc/.  A patch that no longer applies, or a translation unit the harness
does not know, only shows when somebody next builds a variant -- so the tables are checked here
against the source as text.  Nothing is compiled."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tab_variants  # noqa: E402
import wide_variants  # noqa: E402

CSRC = os.path.join(ROOT, "bayesian-consensus-engine_amd", "csrc")
TABLES = {"tab_variants": tab_variants.VARIANTS, "wide_variants": wide_variants.VARIANTS}
ENTRIES = [(t, name) for t, table in TABLES.items() for name in table]


@pytest.mark.parametrize("table,name", ENTRIES)
def test_variant_patch_applies(table, name):
    """Every (file, old, new) of a variant names a file under csrc/ that holds `old`, and the
    replacement changes it."""
    for fn, old, new in TABLES[table][name]:
        path = os.path.join(CSRC, fn)
        assert os.path.isfile(path), f"{table}.{name}: no csrc/{fn}"
        assert old in open(path).read(), f"{table}.{name}: patch text not in csrc/{fn} (stale)"
        assert old != new, f"{table}.{name}: the patch changes nothing"


@pytest.mark.parametrize("module", ["tab_variants", "wide_variants"])
def test_variant_names_are_unique(module):
    """A dict literal keeps the last of two equal keys without a word: count them in the text."""
    text = open(os.path.join(ROOT, "tools", module + ".py")).read()
    body = text[text.index("VARIANTS = {"):]
    body = body[:body.index("\n}\n")]
    names = re.findall(r'^    "(\w+)": \[', body, re.M)
    assert sorted(names) == sorted(TABLES[module]), "the VARIANTS literal and the dict disagree"
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)


def test_variant_build_covers_the_makefile():
    """A variant library links the translation units of csrc/Makefile, all of them."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    cpps = re.search(r"^CPPSRCS := (.*)$", mk, re.M).group(1).split()
    assert list(tab_variants.SRCS) == srcs
    assert list(tab_variants.CPP_SRCS) == cpps
    for fn in srcs + cpps:
        assert os.path.isfile(os.path.join(CSRC, fn)), fn
