import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a HIP (MI355X) device")
    config.addinivalue_line("markers", "slow: multi-process or long-running test")


@pytest.fixture(autouse=True)
def _fresh_quartile_sums():
    """The trainer's quartile sums are process-wide until the next logger dump: a test that
    ends without one must not hand them (on its device) to the next test's trainer."""
    trainer = sys.modules.get("utils.trainer")
    if trainer is not None:
        trainer._QuartileAcc.store.clear()
    yield


def pytest_collection_modifyitems(config, items):
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:  # pragma: no cover
        has_gpu = False
    if has_gpu:
        return
    skip = pytest.mark.skip(reason="no HIP device")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)
