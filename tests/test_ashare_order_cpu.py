"""The launch order of the shared intersections' tasks (build_ashare_plan, option "ashare_inline_warm") without a GPU:
tools/planbench/order_check.cpp plans the headline-shaped group of plan_bench.cpp's bench_ashare (10M docs, 10 000 Zipf
pairs) and the 2 000-query group of tests/test_gpu_ashare_inline_warm.py (1M docs) with the option at 0, 1 and 2 and checks
coverage, the three bands, their doc-slice order, the recorded boundaries, and that option 0 is byte for byte the order of
before the option.  Once more as a ThreadSanitizer build with four planner threads."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "tools", "planbench", "order_check.cpp")
RESIDENT = 1280  # 256 CUs x 5 wavefronts of ashare_kernel: the MI355X grid

SHAPES = [(10_000_000, 10_000), (1_000_000, 2_000)]


def _csrc_objects(B, without=()):
    return [os.path.join(B.OBJ_DIR, os.path.basename(s) + ".o") for s in B.SOURCES
            if os.sep + "csrc" + os.sep in s and os.path.basename(s) not in without]


@pytest.fixture(scope="module")
def order_check(tmp_path_factory):
    from tantivy_amd import build as B

    B.build()  # the kernel objects the planner's translation unit links against
    out = tmp_path_factory.mktemp("order") / "order_check"
    obj = str(out) + ".o"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "-Wno-unused-function", "-fPIC", "-c", SRC, "-o", obj],
                          cwd=str(out.parent))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-o", str(out), obj] + _csrc_objects(B) + ["-ldl", "-lpthread"],
                          cwd=str(out.parent))
    return str(out)


def _modes(stdout):
    """mode -> (warm tasks, independent tasks, leaders with, leaders without, dispatches) from the checker's lines."""
    out = {}
    for m in re.finditer(r"mode (\d): (\d+) tasks, warm (\d+), independent (\d+), leaders with / without warm-up tasks "
                         r"(\d+) / (\d+), bands .*\) (one|two) dispatch", stdout):
        out[int(m.group(1))] = tuple(int(m.group(i)) for i in (3, 4, 5, 6)) + (m.group(7),)
    return out


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("max_doc,n_queries", SHAPES)
def test_bands_cover_order_and_match_the_former_rule(order_check, max_doc, n_queries, threads):
    env = dict(os.environ, TQ_PLAN_THREADS=str(threads), TQ_PLAN_PAR_MIN="1")
    r = subprocess.run([order_check, str(max_doc), str(n_queries), str(RESIDENT)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "order ok" in r.stdout, r.stdout
    modes = _modes(r.stdout)
    assert sorted(modes) == [0, 1, 2], r.stdout
    for warm, indep, with_warm, without, _ in modes.values():
        # the shape has leaders both with and without warm-up tasks: all three bands are populated
        assert warm > 0 and indep > 0 and with_warm > 0 and without > 0, r.stdout
    assert modes[0][4] == "two" and modes[2][4] == "one", r.stdout


def test_a_grid_larger_than_the_independent_band_keeps_the_barrier(order_check):
    """Mode 1 with more resident wavefronts than the batch has independent tasks: two dispatches, the former order."""
    r = subprocess.run([order_check, "1000000", "2000", str(1 << 30)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _modes(r.stdout)[1][4] == "two", r.stdout


def test_order_check_under_thread_sanitizer(tmp_path_factory):
    """The planner translation units and the checker built with -fsanitize=thread, four planner threads: no report."""
    from tantivy_amd import build as B

    B.build()
    d = tmp_path_factory.mktemp("order_tsan")
    csrc = os.path.join(ROOT, "tantivy_amd", "csrc")
    units = ["tq_plan_chunks.cpp", "tq_plan_share.cpp", "tq_plan_misc.cpp"]
    tsan_objs = []
    for src in [os.path.join(csrc, u) for u in units] + [SRC]:
        obj = str(d / (os.path.basename(src) + ".o"))
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC",
                            "-Wno-unused-function", "-fsanitize=thread", "-fno-gpu-sanitize", "-c", src, "-o", obj],
                           capture_output=True, text=True)
        if r.returncode != 0:
            pytest.skip("no ThreadSanitizer build here: " + r.stderr[-300:])
        tsan_objs.append(obj)
    exe = str(d / "order_check_tsan")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-fsanitize=thread", "-fno-gpu-sanitize", "-o", exe] + tsan_objs +
                       _csrc_objects(B, without=units) + ["-ldl", "-lpthread"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("ThreadSanitizer runtime not linkable here: " + r.stderr[-300:])
    env = dict(os.environ, TQ_PLAN_THREADS="4", TQ_PLAN_PAR_MIN="1")
    r = subprocess.run([exe, "1000000", "2000", str(RESIDENT)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ThreadSanitizer" not in r.stdout + r.stderr, (r.stdout + r.stderr)[-2000:]
