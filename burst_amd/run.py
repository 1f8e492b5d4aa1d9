"""Multi-GPU front end: one process per GPU (torchrun), the alignment flags of the burst_hip command line (-r -a -q -o -m -i
-fr -y -k; the taxonomy flags -b*, -w, -t and direct-FASTA references are burst_hip only).

  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
      -m burst_amd.run -r DB.edx -a DB.acx -q reads.fa -o out.b6 -m CAPITALIST -i 0.97 [-fr] [-y]

Every rank loads the database and the queries through the C host (libburst_host.so), aligns its contiguous shard of
unique queries with the C batch scheduler (bh_align_ranges -> libburst_hip.so); every rank's record buffer is a shared-memory
segment rank 0 has mapped (bh_node.c: no collective on the data path, the records cross each rank's own PCIe link behind its
batches), and rank 0 writes the .b6 with the C consolidation code straight from the segments (bh_report_view).  With one process
it is equivalent to burst_hip.
`--shard db` cuts the database instead of the queries (every rank aligns all queries against its clumps; one all_reduce(MIN) of the
per-query minimum -- the launcher's collective handed to bh_search_multi_ex as its reduce_min -- before the same hand-over) for
databases that do not fit one device.
`--samples LIST` in place of -q / -o: a list of query files against the database, which stays on the devices (host.Session); the
ranks walk the list together (run_samples)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np


def read_sample_list(path, taken):
    """[(queries, output), ...] of a --samples list, or (None, exit code) with the reason on standard error: the rules of burst_hip --samples"""
    try:
        lines = open(path).read().split("\n")
    except OSError as e:
        sys.stderr.write("ERROR: Cannot open sample list: %s (%s)\n" % (path, e.strerror))
        return None, 2
    out = []
    for no, ln in enumerate(lines, 1):
        ln = ln.rstrip("\r")
        if not ln or ln.startswith("#"):
            continue
        f = ln.split("\t")
        if len(f) != 2 or not f[0] or not f[1]:
            sys.stderr.write("ERROR: %s line %d: expected 'queries<TAB>output'\n" % (path, no))
            return None, 1
        out.append((f[0], f[1], no))
    if not out:
        sys.stderr.write("ERROR: %s names no sample\n" % path)
        return None, 1
    seen = {}
    for q, o, no in out:
        if o in seen or o in [x[0] for x in out] or o in [t for t in taken if t]:
            sys.stderr.write("ERROR: %s line %d: output '%s' is another line's output or query file, the database, the accelerator or the list itself\n" % (path, no, o))
            return None, 1
        seen[o] = no
    return [(q, o) for q, o, no in out], 0


def open_node_together(host, torch, dist, pdev, rank, world, cap, usable=True):
    """the ranks' shared-memory segments under a fresh job name, opened TOGETHER: rank 0 first (the others map its segment), and if any
    rank cannot have one (/dev/shm too small) every rank hears of it: (node, "") on all ranks, or (None, reason) on all ranks"""
    jt = torch.tensor([int.from_bytes(os.urandom(6), "little") if rank == 0 else 0], dtype=torch.int64, device=pdev)
    dist.broadcast(jt, 0)
    job = "run%x" % int(jt.item())
    node, why = None, ""
    def try_open():
        try:
            return host.Node(job, rank, world, cap), ""
        except host.HostError as e:
            return None, str(e)
    if rank == 0:
        node, why = try_open()
    ok = torch.tensor([1 if (rank != 0 or node is not None) else 0], dtype=torch.int64, device=pdev)
    dist.broadcast(ok, 0)
    if int(ok.item()) and rank != 0:
        node, why = try_open()
    ok = torch.tensor([1 if (node is not None and usable) else 0], dtype=torch.int64, device=pdev)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if not int(ok.item()):
        if node is not None:
            node.close()
        return None, (why or "another rank failed")
    return node, ""


def run_samples(args, samples, db, K, accel, z, rank, local_rank, world, one_dev):
    """--samples: the database stays on the devices (host.Session), the ranks walk the list together.  Per sample: load (the tables
    were parsed on a thread while the previous sample was searched), one all_reduce(MIN) of the status -- a sample that fails on
    any rank fails on all --, the hand-over sized for the largest sample so far (reopened under a fresh job name when a later one
    needs more), the search, rank 0's report, one more all_reduce(MIN).  Usage and I/O errors are the sample's own; any other
    error ends the walk on every rank."""
    import torch
    from burst_amd import host
    dist = None
    if world > 1:
        import torch.distributed as dist
    pdev = "cpu" if one_dev is not None else "cuda"
    exit_of = {host.E_USAGE: 1, host.E_IO: 2, host.E_OOM: 3}
    c0, part = 0, db
    shard_db = args.shard == "db" and world > 1
    if shard_db:
        c0, c1 = host.clump_shard(db, world, rank)
        part = db.slice(c0, c1) if c1 > c0 else None
    build_K = K if args.accelerator_device else 0
    if build_K and world > 1 and not shard_db and not os.environ.get("BURST_HIP_SOLO_BUILD"):
        share = host.dist_share(dist, "cpu" if one_dev is not None else "cuda")
        dev = db.open_device_shared(local_rank, z, build_K, rank, world, share)
    else:
        dev = part.open_device(local_rank, z, build_K=build_K) if part is not None else None
    def agree(rc):
        if world == 1:
            return rc
        t = torch.tensor([rc], dtype=torch.int64, device=pdev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return int(t.item())
    if agree(0 if dev is not None else host.E_USAGE) < 0:
        sys.stderr.write("rank %d: more database shards than clumps\n" % rank)
        if world > 1:
            dist.destroy_process_group()
        return 1
    def reduce_min(a):
        t = torch.from_numpy(a).to(pdev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        a[:] = t.cpu().numpy()
    ses = host.Session(db, dev, mode=args.mode, thres=args.id, rc=args.forwardreverse, z=z, accel=accel, K=K, batch=args.batch, shard_db=world if shard_db else 0,
                       reduce_min=reduce_min if shard_db else None, rank=rank, world=world, c0=c0,
                       coverage=args.coverage, coverage_lengths=args.coverage_lengths, coverage_pad=args.coverage_pad)      # (rank 0's handle: the lines exist only where it reports)
    node, cap_have, first_fail, n_done = None, 0, 0, 0
    ses.prefetch(samples[0][0])
    for i, (q, o) in enumerate(samples):
        t0 = time.time()
        if rank == 0:
            print("Sample %d/%d: %s -> %s" % (i + 1, len(samples), q, o), flush=True)
        if i + 1 < len(samples):
            ses.prefetch(samples[i + 1][0])
        res = ses.load(q, o)
        st = agree(res["rc"])
        if st == 0 and world > 1:
            qs = ses.sample
            u0, u1 = (0, qs.n_uniq) if shard_db else host.shard_range(qs.n_uniq, world, rank)
            strands = 2 if qs.n_entries > qs.n_uniq else 1
            cap = -agree(-(int((u1 - u0) * strands * (4.0 if args.mode in ("FORAGE", "ALLPATHS") else 1.5)) + (1 << 20)))      # (the largest rank's)
            if node is None or cap > cap_have:
                # every rank is past the previous sample (rank 0 has written its report): the old segments may go
                if node is not None:
                    ses.set_node(None)
                    node.close()
                node, why = open_node_together(host, torch, dist, pdev, rank, world, cap)
                if node is None:
                    sys.stderr.write("rank %d: the ranks' shared-memory hand-over could not be set up: %s\n" % (rank, why))
                    ses.drop()
                    st = host.E_OOM
                else:
                    cap_have = cap
                    ses.set_node(node)
                    if rank == 0:
                        print("hand-over: shared-memory segments for %d records per rank" % cap, flush=True)
        if st == 0:
            res = ses.finish()
            st = agree(res["rc"])
        elif res["rc"] == 0:
            ses.drop()                      # (another rank could not have this sample; with --coverage: an all-zero column under its name)
        if st < 0:
            if rank == 0:
                print("Sample %d/%d FAILED (exit code %d): %s" % (i + 1, len(samples), exit_of.get(st, 4), res["err"] or "another rank failed"), flush=True)
            first_fail = first_fail or exit_of.get(st, 4)
            if st not in (host.E_USAGE, host.E_IO) or ses.ended:
                ses.coverage_abort()        # (the error may be another rank's: no tables of a walk that ended early)
                break                       # nothing more is started on a device after a device error
            continue
        n_done += 1
        if rank == 0:
            print("rank 0: %d hit records from %d rank(s) in %.3f s, %d alignments written" % (res["nHits"], world, time.time() - t0, res["nLines"]), flush=True)
    if rank == 0:
        print("Samples: %d done, %d failed" % (n_done, len(samples) - n_done), flush=True)
    if world > 1:
        dist.barrier()
    try:
        ended = ses.ended
        ses.close()      # (with --coverage: rank 0 writes the tables here, unless the walk ended on an error)
        if rank == 0 and args.coverage and not ended and not ses.cov_aborted:
            print("Coverage tables: %s{shared,unique,shared_binary,unique_binary,counts}.txt" % args.coverage, flush=True)
    except host.HostError as e:
        sys.stderr.write("%s\n" % e)
        first_fail = first_fail or 4
    if node is not None:
        node.close()
    if world > 1:
        dist.destroy_process_group()
    return first_fail


def main(argv=None):
    ap = argparse.ArgumentParser(prog="burst_amd.run")
    ap.add_argument("-r", "--references", required=True)
    ap.add_argument("-a", "--accelerator")
    ap.add_argument("-ad", "--accelerator-device", action="store_true", help="no .acx file: the accelerator is built on the devices from the database "
                    "(with several ranks and a replicated database: together, every rank the lists of its share of the words)")
    ap.add_argument("-q", "--queries")
    ap.add_argument("-o", "--output")
    ap.add_argument("--samples", help="in place of -q / -o: a list of query files, one 'queries<TAB>output' per line, aligned one after the other against the "
                    "database, which is read, uploaded and indexed once (host.Session); every rank reads the list, the ranks walk it together")
    ap.add_argument("-m", "--mode", default="CAPITALIST", choices=["BEST", "ALLPATHS", "CAPITALIST", "FORAGE", "ANY"])
    ap.add_argument("-i", "--id", type=float, default=0.97)
    ap.add_argument("-fr", "--forwardreverse", action="store_true")
    ap.add_argument("-y", "--nwildcard", action="store_true")
    ap.add_argument("-k", type=int, default=0, choices=[0, 12, 15], help="accelerator word length (0 = from the file's size)")
    ap.add_argument("--batch", type=int, default=1 << 21)
    ap.add_argument("--shard", default="queries", choices=["queries", "db"],
                    help="queries: database replicated, every rank aligns its range of queries (default); db: every rank holds a "
                         "range of the database's clumps and aligns all queries (for databases larger than one device)")
    ap.add_argument("--coverage", metavar="PREFIX", help="coverage and count tables per reference and sample next to the outputs: "
                    "PREFIX{shared,unique,shared_binary,unique_binary,counts}.txt (computed on rank 0's device from the lines it reports)")
    ap.add_argument("--coverage-lengths", metavar="FILE", help="reference lengths, 'name<TAB>length' per line (default: the database's own extent of every reference)")
    ap.add_argument("--coverage-pad", type=int, default=0, help="bases a placement's range is widened by at both ends")
    ap.add_argument("--mates", help="not available here: paired-end reads are joined by burst_hip --mates (one process, the host gather)")
    ap.add_argument("--cigar", action="store_true", help="not available here: the alignment paths are traced by burst_hip --cigar (one process, the host gather)")
    ap.add_argument("--taxa", metavar="PREFIX", help="not available here: the taxon tables are written by burst_hip --taxa (one process, the host gather)")
    ap.add_argument("--abundance", metavar="PREFIX", help="not available here: the abundance table is written by burst_hip --abundance (one process, the host gather)")
    ap.add_argument("--variants", metavar="PREFIX", help="not available here: the variants table is written by burst_hip --variants (one process, the host gather)")
    ap.add_argument("--cluster", metavar="PREFIX", help="not available here: reads are clustered by burst_hip --cluster (one process, the host gather)")
    ap.add_argument("--cluster-sizes", action="store_true", help="not available here: goes with burst_hip --cluster")
    ap.add_argument("--chimeras", metavar="PREFIX", help="not available here: reads are checked for chimeras by burst_hip --chimeras (one process, the host gather)")
    ap.add_argument("--chimera-sizes", action="store_true", help="not available here: goes with burst_hip --chimeras")
    ap.add_argument("--chimera-skew", metavar="S", help="not available here: goes with burst_hip --chimeras")
    ap.add_argument("--chimera-min-seg", metavar="G", help="not available here: goes with burst_hip --chimeras")
    ap.add_argument("--chimera-min-gain", metavar="D", help="not available here: goes with burst_hip --chimeras")
    ap.add_argument("--sam", action="store_true", help="not available here: SAM records are written by burst_hip --sam (one process, the host gather)")
    ap.add_argument("--sam-unmapped", action="store_true", help="not available here: goes with burst_hip --sam")
    ap.add_argument("--sam-lengths", metavar="FILE", help="not available here: goes with burst_hip --sam")
    ap.add_argument("--consensus", metavar="PREFIX", help="not available here: consensus sequences are written by burst_hip --consensus (one process, the host gather)")
    ap.add_argument("--consensus-min-depth", metavar="N", help="not available here: goes with burst_hip --consensus")
    ap.add_argument("--consensus-min-breadth", metavar="PERMILLE", help="not available here: goes with burst_hip --consensus")
    ap.add_argument("--consensus-reads", metavar="all|unique", help="not available here: goes with burst_hip --consensus")
    ap.add_argument("--consensus-lengths", metavar="FILE", help="not available here: goes with burst_hip --consensus")
    ap.add_argument("--consensus-pairs", action="store_true", help="not available here: goes with burst_hip --consensus")
    ap.add_argument("--consensus-pairs-min", metavar="N", help="not available here: goes with burst_hip --consensus --consensus-pairs")
    ap.add_argument("--vcf", action="store_true", help="not available here: VCF records are written by burst_hip --vcf (one process, the host gather)")
    ap.add_argument("--vcf-min-depth", metavar="N", help="not available here: goes with burst_hip --vcf")
    ap.add_argument("--vcf-min-alt", metavar="N", help="not available here: goes with burst_hip --vcf")
    ap.add_argument("--vcf-reads", metavar="all|unique", help="not available here: goes with burst_hip --vcf")
    ap.add_argument("--vcf-lengths", metavar="FILE", help="not available here: goes with burst_hip --vcf")
    ap.add_argument("--vcf-study", metavar="PREFIX", help="not available here: goes with burst_hip --vcf")
    args = ap.parse_args(argv)
    if args.vcf or args.vcf_min_depth or args.vcf_min_alt or args.vcf_reads or args.vcf_lengths or args.vcf_study:      # (exit code 1, as burst_hip refuses what it cannot do)
        print("ERROR: --vcf is not available in python -m burst_amd.run: use burst_hip --vcf (one process, --gpus N with the host gather)", flush=True)
        return 1
    if args.consensus_pairs or args.consensus_pairs_min:      # (exit code 1, as burst_hip refuses what it cannot do)
        print("ERROR: --consensus-pairs is not available in python -m burst_amd.run: use burst_hip --consensus PREFIX --consensus-pairs (one process, --gpus N with the host gather)", flush=True)
        return 1
    if args.consensus or args.consensus_min_depth or args.consensus_min_breadth or args.consensus_reads or args.consensus_lengths:      # (exit code 1, as burst_hip refuses what it cannot do)
        print("ERROR: --consensus is not available in python -m burst_amd.run: use burst_hip --consensus (one process, --gpus N with the host gather)", flush=True)
        return 1
    if args.sam or args.sam_unmapped or args.sam_lengths:      # (exit code 1, as burst_hip refuses what it cannot do)
        print("ERROR: --sam is not available in python -m burst_amd.run: use burst_hip --sam (one process, --gpus N with the host gather)", flush=True)
        return 1
    if args.chimeras or args.chimera_sizes or args.chimera_skew or args.chimera_min_seg or args.chimera_min_gain:      # (exit code 1, as burst_hip refuses what it cannot do)
        print("ERROR: --chimeras is not available in python -m burst_amd.run: use burst_hip --chimeras (one process, --gpus N with the host gather)", flush=True)
        return 1
    if args.cluster or args.cluster_sizes:      # (exit code 1, as burst_hip refuses what it cannot do)
        print("ERROR: --cluster is not available in python -m burst_amd.run: use burst_hip --cluster (one process, --gpus N with the host gather)", flush=True)
        return 1
    if args.variants:       # (exit code 1, as burst_hip refuses what it cannot do)
        print("ERROR: --variants is not available in python -m burst_amd.run: use burst_hip --variants (one process, --gpus N with the host gather)", flush=True)
        return 1
    if args.taxa:           # (exit code 1, as burst_hip refuses it)
        print("ERROR: --taxa is not available in python -m burst_amd.run: use burst_hip --taxa (one process, --gpus N with the host gather)", flush=True)
        return 1
    if args.abundance:      # (exit code 1, as burst_hip refuses it)
        print("ERROR: --abundance is not available in python -m burst_amd.run: use burst_hip --abundance (one process, --gpus N with the host gather)", flush=True)
        return 1
    if args.mates:
        ap.error("--mates is not available in python -m burst_amd.run: use burst_hip --mates (one process, --gpus N with the host gather)")
    if args.cigar:
        ap.error("--cigar is not available in python -m burst_amd.run: use burst_hip --cigar (one process, --gpus N with the host gather)")
    if (args.coverage_lengths or args.coverage_pad) and not args.coverage:
        ap.error("--coverage-lengths and --coverage-pad go with --coverage PREFIX")
    samples = None
    if args.samples:
        if args.queries or args.output:
            ap.error("--samples names the query files and outputs itself: it does not go with -q / -o")
        samples, code = read_sample_list(args.samples, [args.references, args.accelerator, args.samples])
        if samples is None:
            return code
    elif not args.queries or not args.output:
        ap.error("the following arguments are required: -q/--queries, -o/--output (or --samples)")
    elif args.coverage:
        samples = [(args.queries, args.output)]      # a study of one sample: the session's path
    rank, local_rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    import torch
    one_dev = os.environ.get("BURST_RUN_DEVICE")      # test hook: every rank on this device (gloo plumbing; RCCL refuses two ranks on one device)
    if one_dev is not None:
        local_rank = int(one_dev)
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        if one_dev is not None:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    from burst_amd import host
    z = 0 if args.nwildcard else 1
    if args.accelerator_device and args.accelerator:
        sys.stderr.write("ERROR: -ad builds the accelerator on the device; drop -a\n")
        return 1
    db = host.Db.read(args.references, args.accelerator, K=args.k, z=z)
    K = int(db.c.K) if args.accelerator else (args.k or 12)
    accel = bool(args.accelerator or args.accelerator_device)
    host.lib().bh_queries_sort_device(local_rank)          # large query files are sorted on this rank's own device
    if samples is not None:
        return run_samples(args, samples, db, K, accel, z, rank, local_rank, world, one_dev)
    qs = host.QuerySet(args.queries, args.id, rc=args.forwardreverse, accel=accel, K=K, z=z)
    # the database was sheared for queries up to shear * id long: longer ones would lose alignments across shear boundaries
    # (burst.c:5152-5156: "DB incompatible with selected queries/identity", exit 1)
    if db.c.shear and int(np.float32(qs.c.maxLen) / np.float32(args.id)) > db.c.shear:
        sys.stderr.write("ERROR: DB incompatible with selected queries/identity.\n")
        return 1
    c0 = 0
    part = db
    shard_db = args.shard == "db" and world > 1
    if shard_db:
        c0, c1 = host.clump_shard(db, world, rank)
        part = db.slice(c0, c1) if c1 > c0 else None
    build_K = K if args.accelerator_device else 0
    if build_K and world > 1 and not shard_db and not os.environ.get("BURST_HIP_SOLO_BUILD"):
        # the replicated database's accelerator, built by the ranks together (bhip_build_accelerator_shared); the regions travel over the
        # launcher's process group: in place between the devices under the nccl back end (RCCL), through host memory under gloo
        share = host.dist_share(dist, "cpu" if one_dev is not None else "cuda")
        dev = db.open_device_shared(local_rank, z, build_K, rank, world, share)
    else:
        dev = part.open_device(local_rank, z, build_K=build_K) if part is not None else None
    if dev is not None:
        qs.pin()
    t0 = time.time()
    if world == 1:
        run = host.align_ranges(dev, qs, [(0, qs.n_uniq)], args.mode, args.batch)
        n = host.report(args.output, db, qs, run.hits, args.mode, 0 if accel else host.REP_MERGED_LIST)
        print("rank 0: %d hit records from 1 rank(s) in %.3f s, %d alignments written" % (int(run.c.nHits), time.time() - t0, n))
        return 0
    # several ranks, one process each: the C host's multi-rank search (bh_search_multi_ex), the function behind burst_hip --gpus N.
    # Query-sharded: rank r aligns the r-th share of the unique queries, no collective on the data path.  Database-sharded: every
    # rank aligns all queries against its clumps and the per-query minimum is combined over the ranks -- the launcher's own
    # all_reduce(MIN) (RCCL under the nccl backend) handed to the search as its reduce_min.  Either way every rank's record buffer is
    # a shared-memory segment rank 0 has mapped (bh_node.c) and rank 0 reports from there.
    pdev = "cpu" if one_dev is not None else "cuda"
    u0, u1 = (0, qs.n_uniq) if shard_db else host.shard_range(qs.n_uniq, world, rank)
    strands = 2 if qs.n_entries > qs.n_uniq else 1
    cap = int((u1 - u0) * strands * (4.0 if args.mode in ("FORAGE", "ALLPATHS") else 1.5)) + (1 << 20)
    # the segments are opened TOGETHER: rank 0 first (the others map its segment), and if any rank cannot have one (/dev/shm too small)
    # every rank hears of it and the job ends with the reason on all of them instead of leaving the others in a barrier
    node, why = open_node_together(host, torch, dist, pdev, rank, world, cap, usable=dev is not None or not shard_db)
    if node is None:
        sys.stderr.write("rank %d: the ranks' shared-memory hand-over could not be set up: %s\n" % (rank, why))
        dist.destroy_process_group()
        return 4
    def reduce_min(a):
        t = torch.from_numpy(a).to(pdev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        a[:] = t.cpu().numpy()
    rs = host.RankSearch(dev, rank, world, None, c0=c0, node=node, reduce_min=reduce_min if shard_db else None)
    rs.search(qs, [(u0, u1)], args.mode, args.batch, shard_db=world if shard_db else 0)
    if rank == 0:
        n = host.report_view(args.output, db, qs, rs.view, args.mode, 0 if accel else host.REP_MERGED_LIST)
        print("rank 0: %d hit records from %d rank(s) in %.3f s, %d alignments written" % (int(rs.view.total), world, time.time() - t0, n))
    dist.barrier()      # (the ranks' segments live until rank 0 has written the report)
    rs.close()
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
