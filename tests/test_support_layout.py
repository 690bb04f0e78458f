"""The layout of tests/: restatements and shared helpers live in support modules (``*_ref.py``, ``sim_gpu.py``, ``helpers.py``),
which hold no tests, and no module imports from a test module.  Reads the sources as text."""

import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(HERE, "*.py")))}


def _is_support(name):
    return not name.startswith("test_") and (name.endswith("_ref.py") or name in ("sim_gpu.py", "helpers.py"))


def test_no_module_imports_from_a_test_module():
    pattern = re.compile(r"^\s*(?:from|import)\s+(?:tests\.test_|\.test_|test_)", re.M)
    hits = {name: pattern.findall(text) for name, text in SOURCES.items() if pattern.search(text)}
    assert not hits, hits
    assert not [name for name, text in SOURCES.items() if name != os.path.basename(__file__) and "tests.test_" in text]


def test_support_modules_hold_no_tests():
    support = [name for name in SOURCES if _is_support(name)]
    assert {"relax_ref.py", "md_ref.py", "phonons_ref.py", "sim_gpu.py", "ff_head_ref.py", "helpers.py"} <= set(support)
    pattern = re.compile(r"^(?:def|class)\s+(test_\w*|Test\w*)|^(test_\w*|Test\w*)\s*=", re.M)
    hits = {name: pattern.findall(SOURCES[name]) for name in support if pattern.search(SOURCES[name])}
    assert not hits, hits
