"""Writes tests/golden/synth_default_sha256.json: digests of what the generator writes for the samples of shapes.PIN_SAMPLES when no
shape knob is given.  Run it with the generator binary of the commit whose output is to be kept:
    python tests/golden/make_synth_pin.py path/to/gen_synth_bam
tests/test_random_shapes.py::test_default_files_are_unchanged holds every later generator to these digests (bench.py's input
comes from the same generator)."""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import shapes  # noqa: E402

gen = sys.argv[1]
out = {}
with tempfile.TemporaryDirectory() as td:
    for k, (config, extra) in enumerate(shapes.PIN_SAMPLES):
        pre = Path(td) / f"s{k}"
        subprocess.check_call([gen, "--config", config, "--out", str(pre), *extra], stdout=subprocess.DEVNULL)
        out[shapes.pin_key(config, extra)] = shapes.file_digests(pre)
(HERE / "synth_default_sha256.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
