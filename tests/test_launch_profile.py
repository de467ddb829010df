"""nerf_pytorch_amd.LaunchProfile: parse_report on hand-written reports, the context manager's bookkeeping on the emulator build
(which records nothing), and -- GPU suite, -m gpu -- the counts of a known number of launches of one small kernel."""
import pytest

import nerf_pytorch_amd as N
from nerf_pytorch_amd.launch_profile import parse_report

REPORT = """k_adam 2 0.031250
k_bwd64r<4,true> 3 1.500000
void k_fwd<float, 8> 1 0.250000

k_adam 1 0.018750
k_select_rays 4 0.12"""


def test_parse_report():
    rows = parse_report(REPORT + "\nk_volume_render_fwd 2 0.")       # (a full line: "0." is a float)
    assert rows == {"k_adam": (3, 0.03125 + 0.01875), "k_bwd64r<4,true>": (3, 1.5), "void k_fwd<float, 8>": (1, 0.25),
                    "k_select_rays": (4, 0.12), "k_volume_render_fwd": (2, 0.0)}
    # the tail of a full buffer: cut off in the total, in the count, in the name
    assert parse_report("k_adam 2 0.031250\nk_select_rays 4 0.1e") == {"k_adam": (2, 0.03125)}
    assert parse_report("k_adam 2 0.031250\nk_select_rays 4") == {"k_adam": (2, 0.03125)}
    assert parse_report("k_adam 2 0.031250\nk_sel") == {"k_adam": (2, 0.03125)}
    assert parse_report("") == {} and parse_report("\n\n") == {}


def test_the_emulator_records_nothing(emu):
    with N.LaunchProfile(lib=emu.lib) as prof:
        emu.select_indices(0, 0, 64, 0, 8)
    assert prof.rows == {} and prof.counts() == {} and prof.per_launch(("k_select_indices",), 1) == {}


def test_a_body_that_raises_closes_the_profile(emu):
    with pytest.raises(KeyError, match="from the body"):
        with N.LaunchProfile(lib=emu.lib):
            raise KeyError("from the body")
    with N.LaunchProfile(lib=emu.lib) as prof:      # (profiling was switched off and the open one forgotten)
        pass
    assert prof.rows == {}


def test_nested_entry_is_refused(emu):
    with N.LaunchProfile(lib=emu.lib):
        with pytest.raises(RuntimeError, match="already open"):
            with N.LaunchProfile(lib=emu.lib):
                pass
    with N.LaunchProfile(lib=emu.lib):               # (the refused one did not close the open one's state for good)
        pass


def test_per_launch_and_counts_by_hand():
    prof = N.LaunchProfile()
    prof.rows = {"k_a": (30, 0.45), "k_b": (7, 0.0123456), "k_c": (1, 2.0), "k_none": (0, 0.0)}
    assert prof.counts() == {"k_a": 30, "k_b": 7, "k_c": 1, "k_none": 0}
    # 10 steps: 30 / 10 launches per step, 0.45 ms / 30 = 15 us; 7 / 10, 12.3456 us / 7 = 1.7637 -> 1.76
    assert prof.per_launch(("k_a", "k_b", "k_absent", "k_none"), 10) == {
        "k_a": dict(launches_per_step=3.0, us_per_launch=15.0), "k_b": dict(launches_per_step=0.7, us_per_launch=1.76)}
    assert prof.per_launch(("k_c",), 3) == {"k_c": dict(launches_per_step=0.33, us_per_launch=2000.0)}


@pytest.mark.gpu
def test_launches_of_a_known_kernel_are_counted(gpu):
    def select():
        gpu.select_indices(0, 0, 64, 0, 8)

    with N.LaunchProfile() as prof:
        for _ in range(3):
            select()
    assert list(prof.rows) == ["k_select_indices"]
    launches, ms = prof.rows["k_select_indices"]
    assert launches == 3 and ms > 0
    with N.LaunchProfile() as empty:                 # (the report cleared the records)
        pass
    assert empty.rows == {}
    with pytest.raises(KeyError):
        with N.LaunchProfile():
            select()
            raise KeyError("from the body")
    with N.LaunchProfile() as after:                 # (the discarded block's launch was reported away with it)
        select()
    assert after.counts() == {"k_select_indices": 1}
