"""A loaded sample that the caller gives up (Session.drop: in a job of processes, a sample another rank could not have) is a failed
sample to the coverage: an all-zero column under its name, so that the later samples keep their columns; and a walk that the caller
ends (Session.coverage_abort) writes no tables.  Through the CPU session of tests/test_samples_cpu.py."""
import os

from test_coverage_cpu import EDX, LEN, Q100, Q292, make_align


def walk(tmp_path, abort):
    from burst_amd import host
    db = host.Db.read(EDX)
    seen = {}

    def tap(sample, lines):
        seen[sample] = len(lines)
        return True
    prefix = str(tmp_path / "c_")
    with host.Session(db, None, mode="BEST", thres=0.97, accel=False, align=make_align(db), coverage=prefix, coverage_lengths=LEN, coverage_tap=tap) as s:
        assert s.load(Q100, str(tmp_path / "gone.b6"))["rc"] == 0
        s.drop()
        assert s.run(Q292, str(tmp_path / "kept.b6"))["rc"] == 0 and not s.ended
        sh, un = s.coverage()
        if abort:
            s.coverage_abort()
    db.close()
    return seen, sh, prefix


def test_dropped_sample_is_a_zero_column(tmp_path):
    seen, sh, prefix = walk(tmp_path, False)
    assert sorted(seen) == [1] and seen[1] > 0 and sh.shape[0] == 3            # Dataset, the dropped sample, the kept one
    head = open(prefix + "counts.txt", "rb").read().splitlines()[0]
    assert head == b"#OTU ID\tDataset\tgone\tkept"
    assert not os.path.exists(str(tmp_path / "gone.b6")) and os.path.exists(str(tmp_path / "kept.b6"))


def test_aborted_walk_writes_no_tables(tmp_path):
    walk(tmp_path, True)
    assert sorted(os.listdir(str(tmp_path))) == ["kept.b6"]
