"""Finds the seed list of tests/shapes.py on the CPU: candidate seeds 1, 2, ... in order through shapes.draw, the generator and the
oracle; prints one line per candidate (kept, or why it is dropped) and the first WANT kept seeds at the end.  With --bwa: shapes.draw_bwa and
squid_oracle --bwa, for BWA_SEEDS (WANT defaults to 16).
    python tests/golden/make_shape_seeds.py [--bwa] [WANT [FIRST]]"""
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import oracle_util as ou  # noqa: E402
import shapes  # noqa: E402

BUILD = HERE.parent.parent / "build"
argv = [a for a in sys.argv[1:] if a != "--bwa"]
bwa = "--bwa" in sys.argv[1:]
want = int(argv[0]) if argv else (16 if bwa else 24)
seed = int(argv[1]) if len(argv) > 1 else 1
kept, tried = [], 0
while len(kept) < want:
    gen, flags, _ = shapes.draw_bwa(seed) if bwa else shapes.draw(seed)
    tried += 1
    with tempfile.TemporaryDirectory() as td:
        pre = Path(td) / "s"
        rc, counts = shapes.generate(BUILD, pre, gen)
        why = f"generator exit {rc}" if rc else None
        if not why and bwa:
            orc, sv_path, dump = shapes.run_oracle_bwa(BUILD, pre, td, flags)
            if orc:
                why = f"oracle exit {orc}"
            elif not shapes.usable(sv_path, dump):
                why = "ambiguous order or no call"
            elif not any(not line.startswith("#") for line in (dump / "chimrecord.txt").read_text().splitlines()):
                why = "no rebuilt fragment"
        elif not why:
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
        print(f"seed {seed}: kept  {' '.join(gen[2:])} | {' '.join(flags)} | " + " ".join(f"{k}={counts[k]}" for k in shapes.PLANTED_COUNTS + (("bwa_mapq_below_30",) if "bwa_mapq_below_30" in counts else ())), flush=True)
    seed += 1
print(f"tried {tried}, dropped {tried - len(kept)}")
print("BWA_SEEDS =" if bwa else "SEEDS =", kept)
