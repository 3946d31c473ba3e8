"""The launch stream of the d = 1600 host sequences, call by call, for an A / B of two library builds under
`rocprofv3 --kernel-trace` (one process per build, kernel trace only):
  CMCD_LIB_PATH=<lib> rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/probes/lgcp_launch_stream.py --drive
  python tools/probes/lgcp_launch_stream.py --compare <dir A> <dir B>
--drive runs a fixed list of single calls: the forward and the value-and-gradient call of the cases n20, n33, rc-n33, var-n17,
ula-n20, ulasn-n17, uha-n20, uha-rc-n33 of tests/lgcp_grad_cases.py (dense parameters, the case's form), then the n = 225
forward (the wide path).  Every call stands between two marker launches on a 4099-element tensor: an in-place cosine opens
it, an in-place sine closes it.
--compare cuts each trace at the markers (an opening marker inside an open stretch, or a closing one outside, is an error)
and compares, per call, the ordered list of (kernel name, grid, workgroup size, LDS bytes) of the library's kernels (namespace
cmcd); it prints the launch count of every call and exits 1 on any difference."""
import csv, glob, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASE_IDS = ("n20", "n33", "rc-n33", "var-n17", "ula-n20", "ulasn-n17", "uha-n20", "uha-rc-n33")
WIDE = ("fwd-n225-wide", "MCD_CAIS_sn", 225, 2, 0, {})
CALLS = [(cid, what) for cid in CASE_IDS for what in ("forward", "value+gradient")] + [(WIDE[0], "forward")]


def drive():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import lgcp_grad_cases as lc
    from cmcd_amd import mcdboundingmachine as mcdbm
    marker = torch.zeros(4099, device="cuda")
    for cid, what in CALLS:
        case = WIDE if cid == WIDE[0] else lc.case_by_id(cid)
        mcdbm.KERNEL_VARIANT = case[4]
        b = lc.build(case, "dense")
        seeds = torch.from_numpy(lc.seeds_of(case)).cuda()
        torch.cuda.synchronize()
        marker.cos_()            # opens the call's stretch of the trace (everything the build launched lies before it)
        (lc.forward if what == "forward" else lc.call)(b, seeds)
        torch.cuda.synchronize()
        marker.sin_()            # closes it
        torch.cuda.synchronize()
        print(cid, what, flush=True)


def launches(trace_dir):
    """-> one list per call of (name, grid, workgroup, LDS bytes) in enqueue order."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    cols = rows[0].keys()
    # enqueue order (one host thread: the same in every run), not start order: calls with side streams start out of order
    rows.sort(key=lambda r: int(r["Dispatch_Id"]) if "Dispatch_Id" in cols else int(r["Start_Timestamp"]))
    pick = lambda pat: [c for c in cols if re.fullmatch(pat, c)]
    grid, wg, lds = pick(r"Grid_Size(_[XYZ])?"), pick(r"Workgroup_Size(_[XYZ])?"), pick(r"LDS_Block_Size(_v)?")
    assert grid and wg and lds, list(cols)
    calls, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "cmcd::" not in name:
            opens, closes = "cos_kernel" in name, "sin_kernel" in name       # the markers (torch's elementwise kernels)
            if opens or closes:
                assert opens == (cur is None), "marker out of place: %s at dispatch %s" % (name[:80], r.get("Dispatch_Id"))
                if closes:
                    calls.append(cur)
                cur = [] if opens else None
            continue
        if cur is not None:
            cur.append((re.sub(r"\(.*$", "", name.replace("void ", "")), tuple(int(r[c]) for c in grid), tuple(int(r[c]) for c in wg),
                        int(r[lds[0]])))
    return calls


def compare(dir_a, dir_b):
    a, b = launches(dir_a), launches(dir_b)
    assert len(a) == len(b) == len(CALLS), (len(a), len(b), len(CALLS))
    bad = 0
    for (cid, what), la, lb in zip(CALLS, a, b):
        same = la == lb
        bad += not same
        print("%-14s %-15s launches A %5d, B %5d, distinct kernels %2d: %s"
              % (cid, what, len(la), len(lb), len({l[0] for l in la}), "equal" if same else "DIFFERENT"))
        if not same:
            k = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print("    first difference at launch %d: A %s | B %s" % (k, la[k] if k < len(la) else None, lb[k] if k < len(lb) else None))
    print("LAUNCH STREAMS EQUAL" if not bad else "DIFFERENT CALLS: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--drive":
        drive()
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
