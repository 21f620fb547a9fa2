"""tests/golden/entry_points.txt: what subcommand `entries` of the stand-alone driver program (tests/emul/r2l_entries_lockstep.cpp)
printed when built against the PARENT of the commit that gave the step and static entry points one descriptor and one entering
function each.  Readers of its lines, and the tool that records it:

    python tests/entry_points_record.py <tree>       # <tree>: a `git worktree` of the commit that defines the behaviour

copies this tree's driver sources (test infrastructure; the driver uses the public C ABI only) into <tree>/tests/emul, builds the
program there with the flags of tests/lockstep_driver.py, runs `entries` with no R2L_* variable set and writes the golden file.  It
is regenerated only when behaviour is MEANT to change."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'entry_points.txt')


def text():
    with open(GOLDEN) as f:
        return f.read()


def refusals():
    """{(entry, what is wrong with the call): (code, r2l_last_error())} of the X lines"""
    out = {}
    for line in text().splitlines():
        if line.startswith('X '):
            head, _, tail = line[2:].rpartition(' -> ')
            entry, _, what = head.partition(': ')
            code, _, err = tail.partition(' [')
            out[(entry, what)] = (int(code), err[:-1])
    return out


def flavours():
    """{group: {flavour: digests}} of the F lines"""
    out = {}
    for line in text().splitlines():
        if line.startswith('F ') and not line.startswith('F workspace'):
            group, name, digests = line[2:].split(' | ')
            out.setdefault(group, {})[name] = digests
    return out


def record(tree):
    sys.path.insert(0, HERE)
    import lockstep_driver
    emul = os.path.join(tree, 'tests', 'emul')
    for name in lockstep_driver.DRIVER_SOURCES + ['r2l_lockstep_rt.h']:
        shutil.copy(os.path.join(lockstep_driver.EMUL, name), emul)
    exe = os.path.join(tree, 'tests', 'entries_recorder')
    subprocess.run(['g++', *lockstep_driver.FLAGS, '-I' + emul, os.path.join(emul, 'r2l_lockstep_drivers.cpp'), '-o', exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith('R2L_')}
    r = subprocess.run([exe, 'entries'], capture_output=True, text=True, env=env)
    os.remove(exe)
    if r.returncode or 'runtime error' in r.stderr or 'Sanitizer' in r.stderr:
        sys.exit(r.stderr[-3000:] or f'exit code {r.returncode}')
    with open(GOLDEN, 'w') as f:
        f.write(r.stdout)
    print(f'{GOLDEN}: {len(r.stdout.splitlines())} lines')


if __name__ == '__main__':
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], 'tests', 'emul')):
        sys.exit(__doc__)
    record(sys.argv[1])
