import gzip
import os
import shutil
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TESTS_DIR = os.path.dirname(os.path.abspath(__file__))
# Fixtures recorded from the upstream demo's data tree (config, checkpoints,
# cohort table, the p000194 sample records), laid out as upstream lays them
# out. Files over the committed-size limit are stored gzipped.
GOLDEN_REFERENCE = os.path.join(TESTS_DIR, "golden", "reference")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X GPU")


def pytest_collection_modifyitems(config, items):
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for item in items:
        if "gpu" in item.keywords and not any(
            m in (config.getoption("-m") or "") for m in ("gpu",)
        ):
            item.add_marker(skip)


@pytest.fixture(scope="session")
def reference_dir(tmp_path_factory):
    """The upstream data tree, materialized from tests/golden/reference
    (gzipped members expanded) into a per-session temporary directory."""
    root = str(tmp_path_factory.mktemp("reference"))
    shutil.copytree(GOLDEN_REFERENCE, root, dirs_exist_ok=True)
    for dirpath, _dirs, files in os.walk(root):
        for name in files:
            if name.endswith(".gz"):
                src = os.path.join(dirpath, name)
                with gzip.open(src, "rb") as fi, open(src[:-3], "wb") as fo:
                    shutil.copyfileobj(fi, fo)
                os.remove(src)
    return root
