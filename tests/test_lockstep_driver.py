"""tests/lockstep_driver.py and the program it builds (tests/emul/r2l_lockstep_drivers.cpp): what is not a driver is refused.  The
drivers themselves: test_half_io.py, test_channels_last.py, test_static_half_io.py, test_static_routes.py, test_fwd_routes.py,
test_large_index.py, test_bn_settings.py, test_entry_points.py.  No GPU."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lockstep_driver  # noqa: E402


def test_an_unknown_subcommand_returns_2_and_names_the_eight():
    runs = [lockstep_driver.run('no_such_driver', timeout=60), lockstep_driver.run('half_io_', 'params.bin', timeout=60),
            subprocess.run([lockstep_driver.build()], capture_output=True, text=True, timeout=60)]
    for r in runs:
        assert r.returncode == 2 and r.stdout == '', r.stdout[-2000:] + r.stderr[-2000:]
        assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-3000:]
        listed = [line.split()[0] for line in r.stderr.splitlines()[1:]]
        assert sorted(listed) == sorted(lockstep_driver.SUBCOMMANDS) and len(listed) == 8, r.stderr
