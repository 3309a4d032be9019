"""CPU: the two launch rules of the persistent scan kernels (alp_amd/csrc/persistent_launch.hpp) held directly, without a GPU.  The header is plain C++:
tests/cpp/persistent_launch_test.cpp includes it, is compiled with g++ and prints the grid, or the staging of a sorted list, per row of inputs.  What it must
print is written out here as the launchers had it before the rules were gathered into the header (in_list_kernels.hip, join_kernels.hip,
histogram_kernels.hip, distinct_kernels.hip, quantile_kernels.hip at that commit):
    n_wg = (vectors + waves - 1) / waves;  resident = (n_cus > 0 ? n_cus : 1) * wg_per_cu;
    quantile only: if (max_workgroups != 0 && max_workgroups < resident) resident = max_workgroups;
    grid = n_wg < resident ? n_wg : resident;
    histogram and distinct only: if (tuning grid != 0) grid = tuning grid < 65536 ? tuning grid : 65536;
    stride = n_list > lds_max ? (n_list + lds_max - 1) / lds_max : 1;  n_piv = (n_list + stride - 1) / stride;  lds_max = 32768 / value_bytes"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_MAX = 65536


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    exe = tmp_path_factory.mktemp("persistent_launch") / "persistent_launch_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT}/alp_amd/csrc", "-o", str(exe), f"{ROOT}/tests/cpp/persistent_launch_test.cpp"])

    def run(rows):
        """rows of ("G", 7 inputs) or ("S", 2 inputs) -> one tuple of ints per row"""
        text = "".join(" ".join(str(x) for x in r) + "\n" for r in rows)
        p = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr[-2000:]
        out = [tuple(int(x) for x in line.split()) for line in p.stdout.splitlines()]
        assert len(out) == len(rows)
        return out
    return run


def grid_before(vectors, waves, n_cus, wg_per_cu, max_workgroups=0, tuning_grid=0, grid_max=GRID_MAX):
    n_wg = (vectors + waves - 1) // waves
    resident = (n_cus if n_cus > 0 else 1) * wg_per_cu
    if max_workgroups != 0 and max_workgroups < resident:
        resident = max_workgroups
    grid = n_wg if n_wg < resident else resident
    if tuning_grid != 0:
        grid = tuning_grid if tuning_grid < grid_max else grid_max
    return grid


# (waves per workgroup, n_cus, workgroups per CU) of the five launchers on a 256-CU device, and a small device
SHAPES = [(8, 256, 4), (8, 256, 3), (8, 256, 2), (8, 7, 3), (4, 1, 1)]


def test_the_grid_rule(rules):
    cases = []
    for waves, n_cus, per_cu in SHAPES:
        resident = n_cus * per_cu
        for vectors in (0, 1, waves - 1, waves, waves + 1, resident * waves - 1, resident * waves, resident * waves + 1, (resident + 1) * waves, 1 << 20, (1 << 32) - 1):
            cases.append((vectors, waves, n_cus, per_cu, 0, 0, GRID_MAX))
            cases.append((vectors, waves, 0, per_cu, 0, 0, GRID_MAX))        # n_cus 0 counts as 1
            cases.append((vectors, waves, -3, per_cu, 0, 0, GRID_MAX))
            for override in (0, 1, 5, GRID_MAX - 1, GRID_MAX, GRID_MAX + 1, (1 << 32) - 1):  # 0 is ignored; below, at and above the cap
                cases.append((vectors, waves, n_cus, per_cu, 0, override, GRID_MAX))
            for cap in (0, 1, resident - 1, resident, resident + 1, 1 << 31):  # quantile's max_workgroups: only ever lowers what counts as resident
                cases.append((vectors, waves, n_cus, per_cu, cap, 0, GRID_MAX))
    got = rules([("G",) + c for c in cases])
    bad = [(c, g[0], grid_before(*c)) for c, g in zip(cases, got) if g[0] != grid_before(*c)]
    assert not bad, (len(bad), bad[:5])
    # the named cases once more, as numbers
    by = {c: g[0] for c, g in zip(cases, got)}
    assert by[(0, 8, 256, 4, 0, 0, GRID_MAX)] == 0 and by[(1, 8, 256, 4, 0, 0, GRID_MAX)] == 1
    assert (by[(7, 8, 256, 4, 0, 0, GRID_MAX)], by[(8, 8, 256, 4, 0, 0, GRID_MAX)], by[(9, 8, 256, 4, 0, 0, GRID_MAX)]) == (1, 1, 2)
    assert by[(1024 * 8, 8, 256, 4, 0, 0, GRID_MAX)] == 1024 and by[(1024 * 8 + 1, 8, 256, 4, 0, 0, GRID_MAX)] == 1024
    assert by[(1 << 20, 8, 0, 3, 0, 0, GRID_MAX)] == 3
    assert by[(1 << 20, 8, 256, 3, 0, 5, GRID_MAX)] == 5 and by[(1 << 20, 8, 256, 3, 0, GRID_MAX + 1, GRID_MAX)] == GRID_MAX and by[(0, 8, 256, 3, 0, 5, GRID_MAX)] == 5
    assert by[(1 << 20, 8, 256, 3, 1, 0, GRID_MAX)] == 1 and by[(1 << 20, 8, 256, 3, 769, 0, GRID_MAX)] == 768


@pytest.mark.parametrize("value_bytes", [8, 4])
def test_the_staging_rule(rules, value_bytes):
    lds_max = 32768 // value_bytes
    sizes = [0, 1, lds_max, lds_max + 1, 2 * lds_max, 2 * lds_max + 1, (1 << 31) - 1]
    got = rules([("S", n, value_bytes) for n in sizes])
    for n, (stride, n_piv, got_max) in zip(sizes, got):
        assert got_max == lds_max
        want_stride = (n + lds_max - 1) // lds_max if n > lds_max else 1
        want_piv = (n + want_stride - 1) // want_stride
        assert (stride, n_piv) == (want_stride, want_piv), (n, stride, n_piv)
        assert (stride == 1) == (n <= lds_max)
        assert n_piv == -(-n // stride) and n_piv <= lds_max
        if n > 0:
            assert (n_piv - 1) * stride < n
    assert rules([("S", 0, 2)])[0] == (1, 0, 0)  # neither value size: nothing is held in LDS (the callers pass 8 or 4)
