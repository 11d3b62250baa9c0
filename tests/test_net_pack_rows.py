"""pack_board_rows of tak_amd/csrc/net_pack.h on the CPU, element for element: the weight rows layer 0 of the exact states-entry
towers sums (tower_stage.cuh tower_cb_layer0) — R[plane][tap][O] for the board planes, then a block of −0.0f.

tests/net_pack_rows_host.cpp (its own main, nothing from HIP) fills a folded conv0 from the integer pattern of
tests/net_pack_host.cpp and writes the packer's result.  It is built twice with the host compiler — plain, and with
-fsanitize=address,undefined — and both programs run as child processes; nothing is loaded into Python.  The array is compared with a
numpy slice and transpose of the weights, and must differ from planted index mistakes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tak_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "net_pack_rows_host.cpp")
f32 = np.float32
O, I, BC = 6, 11, 4


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def rows(request, tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("net_pack_rows_" + request.param)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    exe = str(d / "net_pack_rows_host")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, "-I" + CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe, str(d)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    return np.fromfile(str(d / "board_rows"), dtype=f32)


def weights():
    h = (np.arange(O * I * 9, dtype=np.uint64) * 2654435761 + 80 * 40503) & 0xFFFFFFFF
    return ((((h >> 8) & 0xFFFF).astype(np.int64) - 32768) / 256.0).astype(f32).reshape(O, I, 9)


def test_rows_are_the_board_planes_weights_by_plane_then_tap_then_channel(rows):
    w = weights()
    assert rows.shape == ((BC + 1) * 9 * O,)
    R = rows.reshape(BC + 1, 9, O)
    assert np.array_equal(R[:BC], w[:, :BC, :].transpose(1, 2, 0))
    assert len(np.unique(R[:BC])) > 200, "the pattern tells the elements apart"
    # teeth: [tap][plane][O], [plane][O][tap], the planes behind the board planes
    assert not np.array_equal(R[:BC].ravel(), w[:, :BC, :].transpose(2, 1, 0).ravel())
    assert not np.array_equal(R[:BC].ravel(), w[:, :BC, :].transpose(1, 0, 2).ravel())
    assert not np.array_equal(R[:BC], w[:, 1:BC + 1, :].transpose(1, 2, 0))


def test_the_row_of_a_square_without_a_stone_is_minus_zero(rows):
    tail = rows.reshape(BC + 1, 9, O)[BC]
    assert np.all(tail.view(np.uint32) == 0x80000000)
    # what the kernel relies on: adding it changes no bit of any f32, −0.0 and the subnormals included
    x = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x3F800000, 0xBF800001, 0x7F7FFFFF, 0x007FFFFF], np.uint32).view(f32)
    assert np.array_equal((x + tail.ravel()[: len(x)]).view(np.uint32), x.view(np.uint32))
    assert not np.array_equal((x + f32(0.0)).view(np.uint32), x.view(np.uint32))  # +0.0 would turn −0.0 into +0.0
