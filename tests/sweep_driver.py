"""The sweep cells of some length classes on the device, in a process of their own (test_gpu_sweep_variants.py starts it with
BHIP_POISON set, so that every device buffer starts as 0xA5 bytes):
   python tests/sweep_driver.py NW [NW ...]   -- exits non-zero on the first cell whose records or prefix width differ from the oracle's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import sweeplib as sl
from burst_amd import capi


def main(keys):
    n = 0
    for key in keys:
        db = sl.class_db(key)
        devs = {"pairs": capi.Device(db.packed, db.clump_len, db.tot, sl.lut()), "tasks": capi.Device(db.packed, db.clump_len, db.tot, sl.lut(), **db.acx())}
        for cell in sl.CELLS:
            if cell.key != key:
                continue
            dev = devs[cell.feeder]
            for all_hits in (False, True):
                exp = sl.expected(cell, all_hits)
                for band in (1, 0):
                    for k, v in {"two_stage": 1, **cell.options, "band": band}.items():
                        dev.set_option(k, v)
                    got = dev.align_batch(cell.batch(), all_hits=all_hits)
                    st = dev.stats()
                    if got.tobytes() != exp.tobytes() or st["prefix_words"] != cell.nwp:
                        print("MISMATCH", cell.name, "all_hits", all_hits, "band", band, len(got), len(exp), st["prefix_words"])
                        return 1
            n += 1
        for d in devs.values():
            d.close()
    print("sweep driver ok: %d cells" % n)
    return 0


if __name__ == "__main__":
    sys.exit(main([int(a) for a in sys.argv[1:]]))
