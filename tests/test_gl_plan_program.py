"""The Griffin-Lim run planner (csrc/gl_plan.hip) as a stand-alone host program: tests/gl_plan_check.cpp with its own main,
compiled together with the planner as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes
(linked statically: the program needs nothing preloaded) -- and run over its grid of batches.  No GPU, nothing loaded into Python."""
from host_checks import build_and_run


def test_gl_plan_check_program(tmp_path):
    rows, _built = build_and_run('gl_plan_check.cpp', tmp_path, with_csrc=['gl_plan.hip'], timeout=600)
    out = '\n'.join(' '.join(r) for r in rows)
    print(out[-3000:])
    assert ', 0 failures' in out
