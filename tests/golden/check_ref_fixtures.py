"""Check that the committed reference fixtures still regenerate bit for bit from the reference's own code.

    UNIGEN_REFERENCE=<checkout of the reference> python tests/golden/check_ref_fixtures.py

Every generator that executes the reference's code (make_ref_leaf / _wiring / _pipeline) is run into a scratch directory, and each tensor it
writes must equal, bit for bit, the tensor of the same name in the committed fixture; no committed tensor may be missing from the regenerated
file. A fixture that drifted from the reference (or a generator edited without regenerating) fails here instead of silently re-defining what
"the reference says". The reference is not part of this repository, so this runs by hand next to the generators, not in the test suite.
Exits non-zero on the first mismatch.
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import torch
from safetensors import safe_open

HERE = os.path.dirname(os.path.abspath(__file__))
GENERATORS = ("make_ref_leaf_golden.py", "make_ref_wiring_golden.py", "make_ref_pipeline_golden.py")
FIXTURES = ["ref_blocks.safetensors", "ref_leaf.safetensors", "ref_pipeline.safetensors", "ref_wiring.safetensors"]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.uint8) if t.is_floating_point() else t


def main() -> None:
    if not os.path.isdir(os.environ.get("UNIGEN_REFERENCE", "")):
        sys.exit("set UNIGEN_REFERENCE to a checkout of the reference")
    with tempfile.TemporaryDirectory() as td:
        env = dict(os.environ, UG_GOLDEN_OUT=td)
        for gen in GENERATORS:
            r = subprocess.run([sys.executable, os.path.join(HERE, gen)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"{gen} failed: {r.stderr[-800:]}")
        produced = sorted(p for p in os.listdir(td) if p.endswith(".safetensors"))
        if produced != FIXTURES:
            sys.exit(f"the generators wrote {produced}, expected {FIXTURES}")
        for name in produced:
            with safe_open(os.path.join(td, name), "pt") as new, safe_open(os.path.join(HERE, name), "pt") as old:
                if sorted(new.keys()) != sorted(old.keys()):
                    sys.exit(f"{name}: regenerated tensor names differ from the committed fixture")
                for k in old.keys():
                    a, b = new.get_tensor(k), old.get_tensor(k)
                    if not (a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))):
                        sys.exit(f"{name}:{k} differs from the committed fixture")
    print(f"all {len(FIXTURES)} reference fixtures regenerate bit-identically")


if __name__ == "__main__":
    main()
