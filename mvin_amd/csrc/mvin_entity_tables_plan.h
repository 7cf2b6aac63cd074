// The entity tables kernel's deal of jobs to waves, host side and device side from the same functions (mvin_entity_tables.hip).
// A wave owns J consecutive jobs (J weight matrices in its registers) and walks the row tiles once for all of them; a workgroup
// is four waves, so a job group is 4 J consecutive jobs over the same tiles.  Plain C++: tests/test_entity_tables_plan_host.py
// enumerates the deal without HIP.
#pragma once

namespace mvin {

constexpr int kEtWavesPerWg = 4;

// Which instances the library carries: 1 (one matrix per wave, four waves per SIMD) and 2 (two per SIMD).  J = 4 (one wave
// per SIMD on the unified 512-register file) compiles from the same template and was measured: no faster than J = 2
// (profiles/entity_tables_jobs/), so it is not instantiated.
constexpr bool et_jobs_built(int J) { return J == 1 || J == 2; }

// J for a launch of `njobs` jobs.  `forced` is MVIN_ET_JOBS (0: unset; a J that is not built: 1).  Unset: J > 1 only where it
// leaves no wave of a workgroup without work -- 4 J divides the job count -- because a workgroup with idle waves still takes
// its share of the grid cap: measured, the 12-job launch of mvin_key_addressing_flash_prepare and the 4-job launch of
// mvin_fold_tables are slower at J = 2 (126 against 121 us, 59 against 44 us) and the step's 16-job launch faster (145 against
// 156 us).  So 8, 16 and 24 jobs take J = 2 (8 and 24 were not measured: the same full workgroups as 16, half or one and a half
// times as many) and every other count one matrix per wave.
constexpr int kEtBestJobs = 2;
constexpr int et_jobs_per_wave(int njobs, int forced = 0) {
    if (forced > 0) return et_jobs_built(forced) ? forced : 1;
    for (int J = kEtBestJobs; J > 1; J /= 2)
        if (njobs > 0 && njobs % (kEtWavesPerWg * J) == 0) return J;
    return 1;
}

// waves with at least one job, and job groups (the grid's y extent)
constexpr int et_waves(int njobs, int J) { return (njobs + J - 1) / J; }
constexpr int et_groups(int njobs, int J) { return (et_waves(njobs, J) + kEtWavesPerWg - 1) / kEtWavesPerWg; }
// wave w of group g owns jobs [first, first + count): the last wave with work may own fewer than J, the waves behind it none
constexpr int et_wave_first_job(int group, int wave, int J) { return (group * kEtWavesPerWg + wave) * J; }
constexpr int et_wave_job_count(int group, int wave, int njobs, int J) {
    const int left = njobs - et_wave_first_job(group, wave, J);
    return left < 0 ? 0 : left < J ? left : J;
}
// resident workgroups the grid is sized for: 4 / J waves per SIMD on every CU
constexpr int et_wg_cap(int J, int num_cus) { return num_cus * (4 / J); }

}  // namespace mvin
