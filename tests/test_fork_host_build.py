"""csrc/fork/d2d_fork.h (the status rule and the per-row copy of d2d_fork_slots) compiled for the host with gcc as a stand-alone program
under AddressSanitizer and UBSan (tests/csrc/fork_host_main.c + fork_host.c) and run as a child process: every workgroup and thread
of every slot played in turn over heap buffers that end with their last row, on the handmade sets of tests/fork_model.py -- rows of
1 .. 4099 bytes at base offsets 0, 1, 4 and 8, strides that differ from the rows, between two batches and in place -- and on rows
around the cut into runs.  The program prints one digest per item; the numpy model gives the same.  Nothing sanitized is loaded into
this process.  test_gpu_fork_slots.py checks the device build on the same sets."""
import subprocess

import fork_model as FM
import host_build

# rows around D2D_FORK_SMALL_BYTES (one workgroup / eight runs), runs that do not divide, and the search scratch of a slot
EDGE_ROWS = (0, 2, 5, 15, 31, 33, 4095, 4096, 4097, 4100, 4096 + 16 * 8 + 1, 153600)


def cases():
    out = []
    for set_ in (FM.BETWEEN, FM.IN_PLACE):
        out += [(set_, it, k) for k, it in enumerate(FM.case_items(set_))]
        out += [(set_, it, 7 + k) for k, it in enumerate(FM.case_items(set_, rows=EDGE_ROWS, bases=(0, 1, 4)))]
    return out


def test_the_host_program_copies_what_the_model_copies_under_the_sanitizers(tmp_path):
    exe = host_build.sanitized(['fork_host_main.c', 'fork_host.c'], tmp_path, 'fork_host_main')
    todo = cases()
    path = tmp_path / 'cases.txt'
    with open(path, 'w') as f:
        for set_, (n, db, sb, ds, ss), index in todo:
            f.write(' '.join(str(v) for v in [index, set_['in_place'], set_['B_dst'], set_['B_src'], n, db, sb, ds, ss] + set_['src_of']) + '\n')
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split()
    assert len(got) == len(todo) and f'{len(todo)} cases' in run.stderr
    units = set()
    for line, (set_, item, index) in zip(got, todo):
        dst, status = FM.run_case(set_, item, index)
        assert int(line, 16) == FM.digest(dst, status), (set_['in_place'], item, index)
        assert status.tolist() == FM.decide(set_['src_of'], set_['B_src'], set_['in_place']).tolist()
        n, db, sb, ds, ss = item
        for e, s in enumerate(set_['src_of']):
            if status[e] == FM.COPIED:
                diff = (db + e * ds) - (sb + s * ss)
                units.add(16 if diff % 16 == 0 else 4 if diff % 4 == 0 else 1)
    assert units == {1, 4, 16}                  # (the heap is 16-aligned: the offsets decide, and every unit is taken)


def test_the_sets_say_what_the_issue_says():
    assert FM.decide(FM.BETWEEN['src_of'], 3, 0).tolist() == [1, 0, 1, 2, 1]
    assert FM.decide(FM.IN_PLACE['src_of'], 6, 1).tolist() == [0, 1, 0, 1, 2, 2]
