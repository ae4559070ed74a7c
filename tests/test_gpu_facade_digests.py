"""-m gpu: every word the C++ facade produces under a TestSeed is the recorded one, bit for bit.

tests/cpp/facade_digests.cpp drives keys, encryption, decryption, compact results, re-randomisation, the hybrid key switcher and both slot encoders at the
smallest ring the kernels take (N = 256, three data limbs and a special prime, batch 2, t = 65537) and writes each object's words to a file; the SHA-256 of
every file must equal tests/golden/facade_testseed_digests.json.  That file names the commit it was recorded at and is never re-recorded from a branch that
touches the facade: the order in which an entry consumes its generator decides every word here, so any refactor of the facade has to reproduce all of it.

    python tests/test_gpu_facade_digests.py record <commit> [<out.json>]     (on a build of <commit>, with a GPU)
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import pytest

import cpp_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "facade_testseed_digests.json")
LOG2_N, LIMBS = 8, 4    # the fourth prime is the key switcher's special prime

pytestmark = pytest.mark.gpu


def facade_digests(workdir):
    """build tests/cpp/facade_digests.cpp against the tree's libraries, run it, hash what it wrote: name -> SHA-256"""
    from deeppowers_amd.params import ntt_primes
    p = ntt_primes(LOG2_N, LIMBS)
    exe, outdir = cpp_build.build_program("facade_digests"), os.path.join(workdir, "out")
    os.makedirs(outdir)
    args = [exe, outdir, str(LOG2_N)] + [str(v) for q, psi in zip(p.moduli, p.psi) for v in (q, psi)]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "facade digests written" in out.stdout, out.stdout + out.stderr
    digests = {}
    for name in sorted(os.listdir(outdir)):
        with open(os.path.join(outdir, name), "rb") as f:
            digests[name[:-len(".bin")]] = hashlib.sha256(f.read()).hexdigest()
    return digests


def test_testseed_outputs_equal_the_recorded_digests(tmp_path):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = facade_digests(str(tmp_path))
    want = golden["digests"]
    assert sorted(got) == sorted(want)
    differ = [name for name in want if got[name] != want[name]]
    assert not differ, f"differ from the words recorded at {golden['recorded_at']}: {differ}"


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] != "record":
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        recorded = {"recorded_at": sys.argv[2], "log2_n": LOG2_N, "limbs": LIMBS, "digests": facade_digests(tmp)}
    with open(sys.argv[3] if len(sys.argv) > 3 else GOLDEN, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(recorded['digests'])} digests")
