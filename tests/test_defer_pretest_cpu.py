"""fw_defer_pretest.h compiles as plain C++ and its pre-test is conservative: tools/defer_pretest_check.cpp, a short pass (the full one —
1.2e8 ray-box tests under the address and undefined-behaviour sanitizers — is run by hand: profiles/defer_pretest_ab.txt).  The program
exits non-zero if the exact Rect3d test accepts a ray the pre-test rejected, or if the new form lists over 2 % more cornell-like
candidates than the old one."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pretest_admits_every_ray_the_exact_test_accepts(tmp_path):
    exe = str(tmp_path / "defer_pretest_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tools", "defer_pretest_check.cpp")])
    out = subprocess.run([exe, "4e6"], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    assert "new form said no       0 " in out.stdout and out.stdout.rstrip().endswith("OK")
