"""not gpu: every header under gr_amps_amd/csrc compiles on its own -- a translation unit that is nothing but `#include "X"` passes
hipcc's syntax check for gfx950 -- so no header lives on what amps_recc.hip happens to include in front of it.  The one exemption is
recc_chz12_body.hip.h, which is text by design: the body of the filter-bank kernel, included inside each of its two entry points (the
reason stands at its top), and therefore without an include guard."""
import glob
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

from gr_amps_amd import build

TEXT_ONLY = ["recc_chz12_body.hip.h"]
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(build.CSRC, "*.h")))
WORKERS = 4                                            # a compile takes a few seconds; a fixed few side by side, whatever the machine


def _syntax_check(name, tmp):
    tu = os.path.join(tmp, name + ".hip")
    with open(tu, "w") as f:
        f.write('#include "%s"\n' % name)
    r = subprocess.run([build.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-Wno-unused-function",
                        "-I" + os.path.join(build._ROOT, "include"), "-I" + build.CSRC, tu],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout


@pytest.fixture(scope="module")
def checked():
    if not os.path.exists(build.hipcc()):
        pytest.skip("hipcc not installed")
    names = [h for h in HEADERS if h not in TEXT_ONLY]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(WORKERS) as pool:
        return dict(zip(names, pool.map(lambda n: _syntax_check(n, tmp), names)))


def test_the_body_is_the_only_exemption():
    assert TEXT_ONLY == ["recc_chz12_body.hip.h"]
    assert set(TEXT_ONLY) <= set(HEADERS) and len(HEADERS) > len(TEXT_ONLY)
    for name in HEADERS:
        with open(os.path.join(build.CSRC, name)) as f:
            guarded = any(line.strip() == "#pragma once" for line in f)
        assert guarded == (name not in TEXT_ONLY), name


@pytest.mark.parametrize("name", [h for h in HEADERS if h not in TEXT_ONLY])
def test_header_compiles_on_its_own(checked, name):
    rc, out = checked[name]
    assert rc == 0, "%s does not stand alone:\n%s" % (name, out[-2000:])
