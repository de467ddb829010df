"""LaunchProfile: the one place that reads the library's launch profile (include/nerfhip.h: nerfhip_profile_reserve,
nerfhip_profile_enable, nerfhip_profile_report -- every launch between enable(1) and enable(0) is bracketed by two HIP events on its
stream, and the report sums them per kernel name as lines of "name launches total_ms" and clears the records).

    with N.LaunchProfile() as prof:
        engine.step(...)
    prof.rows        # {kernel name: (launches, total_ms)}

The device is synchronised on entry and on exit, and profiling is switched off on exit also when the body raised: a profile left on
would send every later launch of the process through the timed path.  The C side has ONE global record list, so one LaunchProfile
is open at a time.  On the emulator build nothing is recorded: .rows == {}.

bench.py keeps its own spelling of this sequence: it is the yardstick every change is measured with and is not edited, so it is the
one deliberate independent copy.
"""
import ctypes as C

from . import _lib as L

REPORT_BYTES = 1 << 16


def parse_report(text):
    """{kernel name: (launches, total_ms)} of a report's text.  Each line is split from the right into three fields (a name may
    contain spaces); a line without three fields, or whose last two do not parse -- the cut-off tail of a full buffer --, is
    ignored; entries of equal name are summed."""
    rows = {}
    for line in text.splitlines():
        parts = line.rsplit(None, 2)
        if len(parts) != 3:
            continue
        try:
            launches, ms = int(parts[1]), float(parts[2])
        except ValueError:
            continue
        have = rows.get(parts[0], (0, 0.0))
        rows[parts[0]] = (have[0] + launches, have[1] + ms)
    return rows


class LaunchProfile:
    _open = None     # the one that is between __enter__ and __exit__

    def __init__(self, reserve=256, lib=None):
        """reserve: launches to create the events of ahead of the body (event creation stays out of what it times); lib: the
        library to profile (None: the product library)."""
        self.reserve, self.lib, self.rows = reserve, lib, {}

    def _synchronize(self):
        if not self.lib.is_emulated():
            import torch
            torch.cuda.synchronize()

    def __enter__(self):
        if LaunchProfile._open is not None:
            raise RuntimeError("LaunchProfile: one is already open, and the library keeps one global record list")
        if self.lib is None:
            self.lib = L.get_lib()
        self._synchronize()
        self.lib.profile_reserve(self.reserve)
        self.lib.profile_enable(1)
        LaunchProfile._open = self
        return self

    def __exit__(self, *exc):
        try:
            self._synchronize()
        finally:
            LaunchProfile._open = None
            self.lib.profile_enable(0)
            buf = C.create_string_buffer(REPORT_BYTES)
            self.lib.profile_report(buf, len(buf))
            self.rows = parse_report(buf.value.decode())
        return False

    def counts(self):
        """{kernel name: launches}."""
        return {name: launches for name, (launches, _) in self.rows.items()}

    def per_launch(self, names, steps):
        """{name: dict(launches_per_step, us_per_launch)} of the kernels of `names` that were launched, over a body of `steps` steps."""
        return {name: dict(launches_per_step=round(self.rows[name][0] / steps, 2),
                           us_per_launch=round(1000.0 * self.rows[name][1] / self.rows[name][0], 2))
                for name in names if name in self.rows and self.rows[name][0] > 0}
