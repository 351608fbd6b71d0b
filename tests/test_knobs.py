"""Every TSKD_* environment knob the package reads is documented, and every
documented knob is still read: docs/KERNELS.md's knob table == the code."""

import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# TSKD_* names that are read from the environment but are not kernel knobs,
# so the knob table need not list them (it may).
NOT_KERNEL_KNOBS = {"TSKD_CONFIG", "TSKD_GPU_ARCH"}

_READ = re.compile(
    r"""(?:getenv\s*\(|os\.environ(?:\.get\s*\(|\s*\[))\s*["'](TSKD_[A-Z0-9_]+)["']""")


def _knobs_read_by_code():
    names = set()
    for root, _dirs, files in os.walk(os.path.join(REPO, "tskd_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                with open(os.path.join(root, f), encoding="utf-8") as fh:
                    names.update(_READ.findall(fh.read()))
    return names


def _knobs_in_table():
    with open(os.path.join(REPO, "docs", "KERNELS.md"), encoding="utf-8") as fh:
        text = fh.read()
    section = text.split("## Tuning knobs", 1)[1].split("\n## ", 1)[0]
    return set(re.findall(r"^\| `(TSKD_[A-Z0-9_]+)` \|", section, re.M))


def test_knob_table_matches_code():
    code = _knobs_read_by_code()
    table = _knobs_in_table()
    assert code, "no TSKD_* reads found: the scan is broken"
    assert table, "no knob table rows found: the parse is broken"
    assert code - NOT_KERNEL_KNOBS == table - NOT_KERNEL_KNOBS
