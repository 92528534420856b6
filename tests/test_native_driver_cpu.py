"""tests/native_driver.py and tests/cpp/test_support.h held to what the rest of the suite relies on
without saying so: the LCG behind every driver's random cases, the pass criterion of run_driver, and
that the print cap of CHECK hides no failure. Tiny programs written here; no GPU needed."""
import os
import subprocess

import pytest

from native_driver import CPP, build_driver, run_driver

INCLUDE = '#include "%s"\n' % os.path.join(CPP, "test_support.h")


def _program(tmp_path, name, body, seed=None):
    src = tmp_path / (name + ".cc")
    src.write_text(("#define TEST_SUPPORT_SEED %s\n" % seed if seed else "") + INCLUDE + "int main() {\n" + body +
                   '  if (g_fail) { std::printf("%d checks failed\\n", g_fail); return 1; }\n'
                   '  std::printf("ALL OK\\n");\n  return 0;\n}\n')
    return build_driver(src, tmp_path, flags=("-Wall", "-Wextra", "-Werror"))


def _lcg(seed):
    state = seed
    while True:
        state = (state * 6364136223846793005 + 1442695040888963407) % 2**64
        yield (state >> 11) / 2**53


@pytest.mark.parametrize("seed", [None, "20261018ULL"])       # the default, 1, and the seed of three drivers
def test_rnd_and_rndint_are_the_lcg_restated_in_integers(tmp_path, seed):
    out = run_driver(_program(tmp_path, "draws", '  for (int i = 0; i < 4; i++) std::printf("rnd %a\\n", Rnd());\n'
                              '  for (int i = 0; i < 4; i++) std::printf("int %d\\n", RndInt(3, 9));\n', seed))
    draws = _lcg(int(seed[:-3]) if seed else 1)
    assert [float.fromhex(l.split()[1]) for l in out.splitlines() if l.startswith("rnd ")] == [next(draws) for _ in range(4)]
    assert [int(l.split()[1]) for l in out.splitlines() if l.startswith("int ")] == [3 + int(next(draws) * 7) % 7 for _ in range(4)]


def test_run_driver_passes_stdout_on_and_raises_on_a_failed_check(tmp_path, capsys):
    assert "seven\nALL OK\n" == run_driver(_program(tmp_path, "good", '  CHECK(1 + 1 == 2);\n  std::printf("seven\\n");\n'))
    bad = _program(tmp_path, "bad", "  CHECK(1 + 1 == 3);\n")
    with pytest.raises(AssertionError):
        run_driver(bad)
    assert "FAIL " in capsys.readouterr().out            # the driver's own report reaches the test log
    # exit status 0 without the words is no pass either, and neither are the words with a failing status
    silent = tmp_path / "silent.cc"
    silent.write_text("int main() { return 0; }\n")
    with pytest.raises(AssertionError):
        run_driver(build_driver(silent, tmp_path))
    words = tmp_path / "words.cc"
    words.write_text('#include <cstdio>\nint main() { std::printf("ALL OK\\n"); return 3; }\n')
    with pytest.raises(AssertionError):
        run_driver(build_driver(words, tmp_path))


def test_the_print_cap_hides_no_failure(tmp_path):
    exe = _program(tmp_path, "many", "  for (int i = 0; i < 100; i++) CHECK(i < 0);\n")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "ALL OK" not in out.stdout
    assert out.stdout.count("FAIL ") == 40 and "100 checks failed" in out.stdout
