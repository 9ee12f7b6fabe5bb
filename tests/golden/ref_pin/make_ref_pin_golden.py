#!/usr/bin/env python3
"""Records the answers of the two reference pins (tests/test_cli_pin.py, tests/test_ref_pin.py) as data under tests/golden/ref_pin/:
what oracle/_ref/ref_config and oracle/_ref/ref_singlebamrec (oracle/Makefile target `ref`, built from the reference's own sources
where that tree is present) print for every case of the two tests.  The tests compare against these files, and against the
binaries too where they have been built.

    make -C oracle ref && python3 tests/golden/ref_pin/make_ref_pin_golden.py"""
import gzip
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import test_cli_pin  # noqa: E402
import test_ref_pin  # noqa: E402

if not (test_cli_pin.REF.exists() and test_ref_pin.REF.exists()):
    sys.exit("oracle/_ref not built (make -C oracle ref): the committed fixtures are used as they are")
config = [{"argv": argv, "line": test_cli_pin._line([str(test_cli_pin.REF)] + argv)} for argv in test_cli_pin.CASES]
(HERE / "ref_config.json").write_text(json.dumps(config, indent=1) + "\n")
blocks = [{"blocks": b, "answer": test_ref_pin._run(test_ref_pin.REF, b)} for b in test_ref_pin._cases()]
(HERE / "ref_singlebamrec.json.gz").write_bytes(gzip.compress(json.dumps(blocks, sort_keys=True).encode(), mtime=0))
print(f"{len(config)} parser cases, {len(blocks)} block cases written to {HERE}")
