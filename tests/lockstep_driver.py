"""The stand-alone drivers of the lock-step emulation (tests/emul/r2l_lockstep_drivers.cpp: the emulation's sources + the eight
drivers + a main, -fsanitize=address,undefined, no Python in the process): ONE flag list, ONE dependency list, ONE build into
tests/_build/r2l_lockstep_drivers, and run(<subcommand>, ...).  -O0 like the lock-step library: the optimiser needs many minutes
for these sources under the sanitizers.  The library builds of conftest.build_lockstep() are not made here."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
EMUL = os.path.join(HERE, 'emul')
BUILD = os.path.join(HERE, '_build')
EXE = os.path.join(BUILD, 'r2l_lockstep_drivers')
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g']
FLAGS = ['-std=c++17', '-O0', *SANITIZE]
SUBCOMMANDS = ('half_io', 'channels_last', 'static_half', 'static_routes', 'fwd_routes', 'limits', 'bn_settings', 'entries')
DRIVER_SOURCES = ['r2l_lockstep_drivers.cpp', 'r2l_driver_util.h'] + [f'r2l_{name}_lockstep.cpp' for name in SUBCOMMANDS]


def lockstep_deps():
    """what every build of the lock-step emulation's sources depends on"""
    csrc = os.path.join(REPO, 'raw2logit_amd', 'csrc')
    return [os.path.join(EMUL, 'r2l_lockstep.cpp'), os.path.join(EMUL, 'r2l_lockstep_rt.h'),
            os.path.join(REPO, 'include', 'r2l_isp.h')] + [os.path.join(csrc, f) for f in os.listdir(csrc)]


def fresh(target, deps):
    return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in deps)


def build():
    """tests/_build/r2l_lockstep_drivers, rebuilt where a source is newer; -> its path"""
    if not fresh(EXE, [os.path.join(EMUL, f) for f in DRIVER_SOURCES] + lockstep_deps()):
        os.makedirs(BUILD, exist_ok=True)
        tmp = EXE + f'.{os.getpid()}.tmp'
        subprocess.run(['g++', *FLAGS, '-I' + EMUL, os.path.join(EMUL, 'r2l_lockstep_drivers.cpp'), '-o', tmp], check=True)
        os.replace(tmp, EXE)
    return EXE


def run(name, *args, env=None, timeout=900):
    """one driver in a process of its own -> the CompletedProcess (stdout and stderr as text)"""
    return subprocess.run([build(), name, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=env)
