"""Finds the seed list of tests/shapes.py on the CPU: candidate seeds 1, 2, ... in order through shapes.draw, the generator and the
oracle; prints one line per candidate (kept, or why it is dropped) and the first WANT kept seeds at the end.
    python tests/golden/make_shape_seeds.py [WANT [FIRST]]"""
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import oracle_util as ou  # noqa: E402
import shapes  # noqa: E402

BUILD = HERE.parent.parent / "build"
want = int(sys.argv[1]) if len(sys.argv) > 1 else 24
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
kept, tried = [], 0
while len(kept) < want:
    gen, flags, _ = shapes.draw(seed)
    tried += 1
    with tempfile.TemporaryDirectory() as td:
        pre = Path(td) / "s"
        rc, counts = shapes.generate(BUILD, pre, gen)
        why = f"generator exit {rc}" if rc else None
        if not why:
            orc = subprocess.call([str(BUILD / "squid_oracle"), "-b", f"{pre}.bam", "-c", f"{pre}.chim.bam", "-o", str(Path(td) / "oracle"), "--dump", td, *flags],
                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            if orc:
                why = f"oracle exit {orc}"
            elif not shapes.usable(Path(td) / "oracle_sv.txt", Path(td)):
                why = "ambiguous order or no call"
    if why:
        print(f"seed {seed}: dropped, {why}", flush=True)
    else:
        kept.append(seed)
        print(f"seed {seed}: kept  {' '.join(gen[2:])} | {' '.join(flags)} | " + " ".join(f"{k}={counts[k]}" for k in shapes.PLANTED_COUNTS), flush=True)
    seed += 1
print(f"tried {tried}, dropped {tried - len(kept)}")
print("SEEDS =", kept)
