"""Key32<float>: the compare-free key of the fill's raster kernels (to_fold) equals the key by selects (to) for every
non-NaN bit pattern, and from() inverts it.  All 2^32 patterns, on the host: tests/cpp/key32_exhaustive.cpp, built with the
library's floating-point flags.  About ten seconds; the device side of the same claim is tests/test_fill_interior_paths_gpu.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fold_key_equals_select_key_for_every_bit_pattern():
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-C", cpp, "-f", "Makefile.key32", "key32_exhaustive"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(cpp, "key32_exhaustive")], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout
    assert "4278190082 non-NaN patterns checked, 0 differ" in r.stdout     # 2^32 less the 2 * (2^23 - 1) NaN patterns
