"""No GPU: the entity tables kernel's deal of jobs to waves (mvin_amd/csrc/mvin_entity_tables_plan.h, plain C++ shared by the
launcher and the kernel).  A stand-alone program (its own main, built with the address and undefined-behaviour sanitizers, never
loaded into Python) enumerates it for 1 .. 24 jobs and every J: each job is owned by exactly one wave, no wave owns more than J,
the waves with work fill the job groups the grid's y extent counts, and the J the launcher picks by itself is a built one that
leaves no wave of a workgroup idle."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvin_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "mvin_entity_tables_plan.h"

using namespace mvin;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d (njobs %d, J %d): %s\n", __LINE__, njobs, J, #c); return 1; } } while (0)

int main() {
    for (int njobs = 1; njobs <= 24; ++njobs) {
        for (int J : {1, 2, 4}) {                                // (4: the deal holds for it too, built or not)
            CHECK(et_jobs_per_wave(njobs, J) == (et_jobs_built(J) ? J : 1));      // the switch is obeyed for every built J
            const int groups = et_groups(njobs, J);              // the grid's y extent
            CHECK(groups >= 1 && (groups - 1) * kEtWavesPerWg * J < njobs && njobs <= groups * kEtWavesPerWg * J);
            int owners[24] = {};
            int busy = 0;
            for (int g = 0; g < groups; ++g)
                for (int w = 0; w < kEtWavesPerWg; ++w) {
                    const int first = et_wave_first_job(g, w, J), n = et_wave_job_count(g, w, njobs, J);
                    CHECK(n >= 0 && n <= J);
                    CHECK(n == 0 || first + n <= njobs);
                    CHECK(n == J || first + n >= njobs);         // only the last wave with work owns fewer than J
                    busy += n > 0;
                    for (int j = first; j < first + n; ++j) ++owners[j];
                }
            for (int j = 0; j < njobs; ++j) CHECK(owners[j] == 1);
            CHECK(busy == et_waves(njobs, J));
            CHECK(et_wave_job_count(groups, 0, njobs, J) == 0);  // and a group past the grid would own nothing
        }
        int J = et_jobs_per_wave(njobs);                          // the launcher's own choice
        CHECK(et_jobs_built(J));
        CHECK(J == 1 || njobs % (kEtWavesPerWg * J) == 0);
        J = 3;
        CHECK(et_jobs_per_wave(njobs, 3) == 1 && et_jobs_per_wave(njobs, 4) == 1 && et_jobs_per_wave(njobs, 8) == 1);     // a J that is not built: one matrix per wave
    }
    int njobs = 16, J = et_jobs_per_wave(16);
    CHECK(J == kEtBestJobs);                                     // the step's 16-job launch takes the measured best
    CHECK(et_wg_cap(1, 256) == 1024 && et_wg_cap(2, 256) == 512 && et_wg_cap(4, 256) == 256);
    std::printf("OK\n");
    return 0;
}
"""


def _cxx():
    for cand in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and (os.path.exists(cand) or shutil.which(cand)):
            return cand
    return None


def test_every_job_has_one_wave_and_no_wave_more_than_J(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "entity_tables_plan.cpp"
    exe = tmp_path / "entity_tables_plan"
    src.write_text(PROGRAM)
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          f"-I{CSRC}", str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip() == "OK", res.stdout + res.stderr
