"""examples/decode_subband.py, run the way tests/test_c_example.py runs the other examples: system A's 21 reverse control channels out
of one 800 ksps stream through the shared translate seam.  Without a GPU it must say so and leave with an error -- there is no CPU path
behind the ABI; on the MI355X every burst comes back with the MIN that was sent (the script's own exit code)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "examples", "decode_subband.py")


def test_subband_example_refuses_to_run_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is here: the run is test_python_example_of_the_shared_translate_seam")
    p = subprocess.run([sys.executable, SCRIPT], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 1 and "no CPU fallback" in p.stderr, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])


@pytest.mark.gpu
def test_python_example_of_the_shared_translate_seam(gpu):
    p = subprocess.run([sys.executable, SCRIPT], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert "21 bursts sent, 21 decoded" in p.stdout and "MISMATCH" not in p.stdout
    assert p.stdout.count("  MIN ") == 21
