"""The tail queue's plan and ticket rules (csrc/tail_queue.h), executed on the CPU.

tests/tail_queue_recorder.hip is a host-only build of the header the kernels include: the plan (how many tiles stay static, how many
go by ticket, the grid), the static walks with S in place of the grid size, the ticket -> tile rule, who zeroes the counter, and the
grouped launch's tile -> problem lookup.  Whatever the order in which the workgroups past S draw their tickets (each draws exactly
one, the atomic hands every value out once), every tile of the launch must be produced exactly once, the spare workgroups must
produce none, and exactly one workgroup -- the drawer of the last ticket -- must reset the counter."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orbit-2_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tailq") / "tail_queue_recorder")
    subprocess.run([HIPCC, "--offload-host-only", "-std=c++17", "-O1", "-w", "-I", CSRC,
                    os.path.join(ROOT, "tests", "tail_queue_recorder.hip"), "-o", exe], check=True, capture_output=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return r.stdout.splitlines()
    return run


def _plan(T, tail):
    """the rule of DESIGN 4.12, written down a second time: S = T - tail, grid = S + 2 tail; anything else is static"""
    if tail <= 0 or tail > T:
        return T, 0, T
    return T - tail, tail, T + tail


def _orders(n, rng):
    """ticket orders for n drawing workgroups: in order, reversed, the spare half first, and random ones"""
    ident = list(range(n))
    out = [ident, ident[::-1], ident[n // 2:] + ident[:n // 2]]
    for _ in range(3):
        p = ident[:]
        rng.shuffle(p)
        out.append(p)
    return out


def _check_launch(out, T, tail, ends=None):
    """out: the recorder's three lines for one `sim`.  Every tile once, spares none, one reset by the last ticket's drawer."""
    S, tl, grid = (int(v) for v in out[0].split())
    assert (S, tl, grid) == _plan(T, tail)
    tiles = out[1].split()[1:]
    assert out[1].startswith("tiles:") and len(tiles) == grid
    produced = [t for t in tiles if t != "-1"]
    if ends:
        want, first = [], 0
        for pi, e in enumerate(ends):
            want += ["%d:%d" % (pi, i) for i in range(e - first)]
            first = e
    else:
        want = [str(i) for i in range(T)]
    assert sorted(produced) == sorted(want)                       # every tile exactly once
    assert len(produced) == T and tiles.count("-1") == grid - T == tl            # the spare workgroups produce none
    assert all(t != "-1" for t in tiles[:S])                      # static workgroups never return empty-handed
    return S, tl, grid, tiles, [int(v) for v in out[2].split(":")[1].split()]


def _sim(recorder, cases):
    """cases: (walk, T, tail, ends or None, tickets) -> the checked result of each"""
    lines = []
    for walk, T, tail, ends, tickets in cases:
        ln = "sim walk=%s T=%d tail=%d tickets=%s" % (walk, T, tail, ",".join(map(str, tickets)))
        lines.append(ln + (" ends=" + ",".join(map(str, ends)) if ends else ""))
    out = recorder(lines)
    assert len(out) == 3 * len(cases)
    res = []
    for i, (walk, T, tail, ends, tickets) in enumerate(cases):
        S, tl, grid, tiles, resets = _check_launch(out[3 * i:3 * i + 3], T, tail, ends)
        if tl:
            assert resets == [S + tickets.index(2 * tl - 1)]      # the drawer of the last ticket, nobody else
            for i_wg, t in enumerate(tickets):                     # ticket t < tail is tile S + t
                if not ends:
                    assert tiles[S + i_wg] == (str(S + t) if t < tl else "-1")
        else:
            assert resets == []
        res.append((S, tl, grid))
    return res


def test_plan_rules(recorder):
    cases = [(0, 0), (1, 0), (1, 1), (1, 2), (320, 64), (320, 320), (320, 321), (320, -5), (1728, 512), (12288, 512), (100, 512),
             (2 ** 31 - 1, 512), (2 ** 31 - 600, 512), (2 ** 30, 2 ** 30), (2 ** 30 + 5, 2 ** 30)]
    out = recorder(["plan T=%d tail=%d" % c for c in cases])
    for (T, tail), ln in zip(cases, out):
        S, tl, grid = (int(v) for v in ln.split())
        want = _plan(T, tail) if T + max(tail, 0) <= 2 ** 31 - 1 else (T, 0, T)     # a grid past 2^31 - 1 is never planned
        assert (S, tl, grid) == want, (T, tail)
        assert S + tl == T and grid == S + 2 * tl and grid <= 2 ** 31 - 1


def test_entry_argument_rules(recorder):
    """the entry points' `tail`: 0 = whole rounds of the device's slots when at least 4 rounds stay static, > 0 = forced, < 0 = static;
    slots = 0 (not the 256-CU / 8-XCD part) is always static"""
    cases = [(12288, 0, 2, 256, 512), (1536, 0, 2, 256, 512), (1535, 0, 2, 256, 0), (1728, 0, 2, 256, 512), (320, 0, 2, 256, 0),
             (12288, 0, 2, 0, 0), (12288, 0, 0, 256, 0), (12288, -1, 2, 256, 0), (320, 64, 2, 256, 64), (320, 64, 2, 0, 64),
             (320, 400, 2, 256, 0), (12288, 0, 3, 304, 912), (12288, 0, 1, 256, 256)]
    out = recorder(["arg T=%d tail_arg=%d rounds=%d slots=%d" % c[:4] for c in cases])
    for (T, arg, rounds, slots, want_tail), ln in zip(cases, out):
        assert tuple(int(v) for v in ln.split()) == _plan(T, want_tail), (T, arg, rounds, slots)


@pytest.mark.parametrize("walk", ["round", "range"])
def test_every_tile_once_for_any_ticket_order(recorder, walk):
    rng = random.Random(20260 + len(walk))
    grids = [(320, 64), (384, 128), (256, 256), (257, 1), (1, 1), (7, 3), (300, 44), (1000, 300), (1728, 512), (2049, 512)]
    grids += [(T, rng.choice([1, 8, 64, 256, 512, max(1, T // 3), T])) for T in (rng.randrange(1, 3000) for _ in range(12))]
    grids += [(T, T + rng.randrange(1, 600)) for T in (rng.randrange(1, 700) for _ in range(4))]      # tails larger than T: static
    grids += [(256 * r + o, t) for r, o, t in ((1, 17, 64), (3, 255, 256), (5, 1, 512), (2, 128, 200))]   # T no multiple of 256
    cases = []
    for T, tail in grids:
        n = 2 * tail if 0 < tail <= T else 0
        for order in (_orders(n, rng) if n else [[]]):
            cases.append((walk, T, tail, None, order))
    res = _sim(recorder, cases)
    assert any(tl == 0 for _, tl, _ in res) and any(tl > 0 and S % 256 for S, tl, _ in res)


def test_grouped_launches(recorder):
    """2 to 12 problems in one grid: the tile -> problem lookup sees every local tile of every problem once, wherever the tail
    starts (inside a problem, on a problem's edge, spanning several small problems)"""
    rng = random.Random(812)
    cases = []
    for n in range(2, 13):
        sizes = [rng.choice([1, 4, 12, 48, 144, 576]) for _ in range(n)]
        ends = [sum(sizes[:i + 1]) for i in range(n)]
        T = ends[-1]
        for tail in {1, min(T, 64), min(T, 256), sizes[-1], min(T, sizes[-1] + sizes[-2]), T, T + 9}:
            k = 2 * tail if tail <= T else 0
            for order in (_orders(k, rng)[2:5] if k else [[]]):
                cases.append(("round", T, tail, ends, order))
    # the Block's balanced weight-gradient group at interm_1b: 3 full problems (1536 tiles), 2 x 4 quarter-length ones (768)
    ends = [576, 1152, 1536] + [1536 + 96 * (i + 1) for i in range(8)]
    cases.append(("round", 2304, 512, ends, _orders(1024, rng)[5]))
    _sim(recorder, cases)
