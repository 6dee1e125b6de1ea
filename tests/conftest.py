import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


# Under pytest-xdist every worker that has run a GPU test keeps the GPU open, and several tests start one more GPU process of their
# own (subprocess.run, one at a time).  A GPU serves at most 16 processes: at most MAX_WORKERS workers keep the suite at half of that
# however many CPUs `-n auto` finds or `-n N` asks for.
MAX_WORKERS = 4


@pytest.hookimpl(tryfirst=True)
def pytest_cmdline_main(config):
    if getattr(config.option, "numprocesses", None) is not None:  # (pytest-xdist is loaded; its own hook resolves -n after this one)
        config.option.maxprocesses = min(config.option.maxprocesses or MAX_WORKERS, MAX_WORKERS)


SESSION_T0 = __import__("time").time()  # tests/test_zz_full_grid_parity.py sizes its CPU-side budgets against the suite's elapsed time
