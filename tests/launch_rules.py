"""Python restatement of the engine's admission rules for the launch forms that need co-resident workgroups (csrc/engine.cpp:
udt_blocked_fits, sweep_fused_fits, wrap_one_launch; csrc/qr.hip: qr_coop_grid), fed with the capacities
dqmc_launch_plan reports.  A unit is one walker x one block; the block maps launch whole groups of eight units."""


def ceil8(units):
    return (units + 7) // 8 * 8


def capacities(gpu):
    """[CUs, workgroups of the one-launch UDT, of the cooperative QR, of the one-launch wrap without / with a pending chunk]
    from a one-walker 16 x 16 handle, which every form admits"""
    mc = gpu.DQMC(gpu.HubbardModelAttractive(16, 2), beta=1.0, n_walkers=1, seed=1)
    plan = mc.launch_plan()
    assert mc.kron_hopping()
    mc.close()
    assert plan["units"] == 1 and plan["units_padded"] == 8
    caps = dict(cus=plan["cus"], udt_blocks=plan["udt_blocks"], qr_coop_blocks=plan["qr_coop_blocks"],
                wrap_blocks=plan["wrap_blocks"])
    assert caps["cus"] > 0 and caps["udt_blocks"] % caps["cus"] == 0 and caps["qr_coop_blocks"] % caps["cus"] == 0
    return caps


def udt_one_launch(n, units, caps):
    """eight workgroups per unit, all co-resident; n = 256 only"""
    return n == 256 and caps["udt_blocks"] > 0 and ceil8(units) * 8 <= caps["udt_blocks"]


def qr_coop(n, units, caps):
    """eight workgroups per unit, all co-resident; n <= 256"""
    return n <= 256 and ceil8(units) * 8 <= caps["qr_coop_blocks"]


def sweep_fused(n, walkers, nb, caps):
    """one elimination workgroup per walker beside the flush workgroups of the previous chunk, one workgroup per CU"""
    if n % 64 != 0 or n < 128:
        return False
    ncp = 2 if n % 256 == 0 else 1
    nt = 8 if n % 128 == 0 else 4
    flush_blocks = ceil8(walkers * nb) * (n // 64) * (n // (16 * nt * ncp))
    return walkers + flush_blocks <= caps["cus"]


def wrap_one_launch(factored, units, caps):
    """sixteen workgroups per unit, all co-resident, asked without / with a pending sweep chunk"""
    return tuple(int(factored and ceil8(units) * 16 <= caps["wrap_blocks"][pf]) for pf in (0, 1))


def expected_plan(n, walkers, nb, factored, caps):
    """what dqmc_launch_plan must report for a handle without kernel switches"""
    units = walkers * nb
    one = udt_one_launch(n, units, caps)
    return dict(units=units, units_padded=ceil8(units), cus=caps["cus"], udt_sites=7 if one else 0,
                udt_blocks=caps["udt_blocks"] if one else 0, qr_coop_blocks=caps["qr_coop_blocks"] if n <= 256 else 0,
                qr_coop=int(qr_coop(n, units, caps)), sweep_fused=int(sweep_fused(n, walkers, nb, caps)),
                wrap_blocks=tuple(caps["wrap_blocks"]) if factored else (0, 0),
                wrap_one_launch=wrap_one_launch(factored, units, caps))


def forms(plan, n):
    """the forms a handle with this plan runs: (UDT, site sweep, wrap without / with a pending chunk)"""
    if plan["udt_sites"] == 7:
        udt = "one_launch"
    elif plan["qr_coop"]:
        udt = "coop"
    else:
        udt = "tile" if n == 256 else "single"
    return udt, "fused" if plan["sweep_fused"] else "split", tuple(plan["wrap_one_launch"])


def regimes(plan, n, factored):
    """the conditions of the regime list (tests/test_gpu_unit_counts.py) that a handle with this plan meets"""
    udt, sweep, wrap = forms(plan, n)
    units = plan["units"]
    r = set()
    if udt == "one_launch" and units > 8 and units % 8 != 0:
        r.add("one-launch UDT with a partial later group")
    if udt == "coop" and n == 256:
        r.add("cooperative QR with %s sweep" % sweep)
        if plan["units_padded"] * 8 == plan["qr_coop_blocks"]:
            r.add("cooperative QR at its admitted maximum")
    if udt == "tile":
        r.add("tile QR")
    if factored:
        if wrap == (1, 1):
            r.add("one-launch wrap")
        elif wrap == (0, 0):
            r.add("two-launch wrap")
        else:
            r.add("mixed wrap forms")
    return r


def mixed_wrap_units(caps):
    """unit counts whose handle takes one wrap form without and the other with a pending chunk (empty if none)"""
    lo, hi = sorted(b // 16 for b in caps["wrap_blocks"])
    return [u for u in range(1, hi + 1) if lo < ceil8(u) <= hi]
