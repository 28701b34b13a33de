"""Import a config script (configs/NAME.py) as its ``__main__`` would run it, with a command line of the test's."""
from __future__ import annotations

import importlib
import sys
from pathlib import Path

CONFIGS = Path(__file__).resolve().parents[1] / "configs"


def load_config(monkeypatch, script: str, argv):
    """The module of configs/``script``.py, freshly imported with ``argv`` as its command line.  The scripts read the
    command line and build their factories on import, so neither the script nor configs/_common.py stays imported."""
    monkeypatch.setattr(sys, "argv", [f"{script}.py", *argv])
    monkeypatch.syspath_prepend(str(CONFIGS))
    for m in ("_common", script):
        sys.modules.pop(m, None)
    try:
        return importlib.import_module(script)
    finally:
        for m in ("_common", script):
            sys.modules.pop(m, None)
