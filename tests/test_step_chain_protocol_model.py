"""CPU: an executable model of rowstep_kernel's hand-off protocol (acezero_amd/csrc/head_kernels.hip: rowstep_kernel,
rowseq_loss_stage, rowseq_layers on head_seq.h's seq_seams, seq_bump, seq_catch_up and SEQ_DEAD; head_api.hip: launch_rowstep,
seq_account), in the style of tests/test_seq_protocol_model.py. One launch runs, per
row tile, the forward layers, the loss blocks and the input-gradient layers on the tile's four workgroups; every stage but the last
bumps the tile's counter 8 times per workgroup (a layer: eight waves, one each; the loss stage: eight waves x 1 in column tile 0, four
waves x 2 in the others), and every stage but the first polls it:
    forward layer k > 0       (base + k) * 32
    loss blocks               (base + n_fwd) * 32            the last forward layer signals too
    input-gradient layer j    (base + n_fwd + 1 + j) * 32
which makes n_fwd + n_bwd seams per launch (15 for the default head). The model checks, over tile counts 1, 2, 9 and 64 and random
wave-level interleavings, that a poll can only be passed once ALL producers of its seam have signalled (its target lies strictly above
every value the counter can hold before that), that a dead launch adds exactly a live launch's amount, that workgroups without a row
tile touch nothing, and that steps of the merged and the three-launch flow interleaved leave counters and host bases in step."""
import random

import pytest

N_FWD, N_BWD = 8, 7
TILE_COUNTS = [1, 2, 9, 64]


def decode(block, mtiles):
    per_xcd = (mtiles + 7) >> 3
    jx = block >> 3
    mt = (block & 7) * per_xcd + (jx >> 2)
    return None if mt >= mtiles else (block & 7, mt, jx & 3)


def stages(kind):
    """The stages a workgroup runs in a launch of this kind and the seams of the launch in front of the first of them:
    (name, polls, signals). Seam s of the launch is signalled by the stage in front of it and polled by the stage behind it."""
    fwd = [("fwd%d" % k, k > 0, True) for k in range(N_FWD)]
    bwd = [("bwd%d" % j, True, j + 1 < N_BWD) for j in range(N_BWD)]
    if kind == "fwd":        # rowseq_kernel<false>: the last layer does not signal
        return fwd[:-1] + [("fwd%d" % (N_FWD - 1), True, False)]
    if kind == "loss_bwd":   # rowseq_loss_kernel: the loss blocks read what an earlier launch wrote
        return [("loss", False, True)] + bwd
    assert kind == "step"    # rowstep_kernel
    return fwd + [("loss", True, True)] + bwd


def seams(kind):
    return sum(1 for _, _, signals in stages(kind) if signals)


class Device:
    def __init__(self):
        self.flags = [0] * 64
        self.base = [0] * 64
        self.touched = set()

    def launch(self, kind, mtiles, rng, active=True):
        st = stages(kind)
        base = list(self.base)                                  # the kernel argument: a snapshot
        for mt in range(mtiles):
            self.base[mt] += seams(kind)                        # launch_rowseq / launch_rowstep
        wgs = [d for d in map(lambda b: decode(b, mtiles), range(32 * ((mtiles + 7) // 8))) if d]
        assert len(wgs) == 4 * mtiles and len({(mt, nt) for _, mt, nt in wgs}) == 4 * mtiles
        for xcd, mt, _ in wgs:                                  # the four column tiles of a row tile share an XCD
            assert all(x == xcd for x, m, _ in wgs if m == mt)
        self.touched |= {mt for _, mt, _ in wgs}
        if not active:                                          # the entry test: one add per workgroup
            for _, mt, _ in wgs:
                self.flags[mt] += 8 * seams(kind)
            return
        # waves: [mt, nt, wave, stage index, signalled]; a loss stage is run by eight waves in column tile 0 and by four in the others
        waves = [[mt, nt, w, 0] for _, mt, nt in wgs for w in range(8)]
        finished = {}                                           # (mt, stage index) -> signals of that stage so far (of 32)
        while waves:
            wv = rng.choice(waves)
            mt, nt, w, si = wv
            name, polls, signals = st[si]
            runs = name != "loss" or nt == 0 or w < 4           # the loader waves of column tiles 1..3 gather instead
            seam = sum(1 for s in st[:si] if s[2])              # seams of this launch in front of the stage
            if polls and runs:
                target = (base[mt] + seam) * 32
                if self.flags[mt] < target:
                    continue                                    # polling
                assert finished.get((mt, si - 1), 0) == 32, (kind, mt, name)   # every producer has signalled
            elif polls and name != "loss":
                raise AssertionError("only the loss stage has waves that skip it")
            if signals and runs:
                inc = 2 if (name == "loss" and nt != 0) else 1
                # strictly below every later target until the last signal of this seam is in
                assert self.flags[mt] + inc <= (base[mt] + seam + 1) * 32
                self.flags[mt] += inc
                finished[(mt, si)] = finished.get((mt, si), 0) + inc
            wv[3] += 1
            if wv[3] == len(st):
                waves.remove(wv)


def test_fifteen_seams_per_launch():
    assert seams("step") == N_FWD + N_BWD == 15
    assert seams("fwd") + seams("loss_bwd") == seams("step") - 1   # the forward -> loss seam is the one a kernel boundary used to be
    # the poll targets of a launch, in stage order, are base + 1 .. base + 15: each seam is polled exactly once
    st = stages("step")
    targets = [sum(1 for s in st[:i] if s[2]) for i, s in enumerate(st) if s[1]]
    assert targets == list(range(1, 16))


@pytest.mark.parametrize("mtiles", TILE_COUNTS)
def test_no_stage_starts_before_its_producers_and_counters_keep_step(mtiles):
    rng = random.Random(mtiles)
    dev = Device()
    for _ in range(3):
        dev.launch("step", mtiles, rng)
    assert all(dev.flags[mt] == 32 * dev.base[mt] == 32 * 45 * (mt < mtiles) for mt in range(64))
    assert dev.touched == set(range(mtiles))                    # workgroups without a row tile leave every counter alone


@pytest.mark.parametrize("mtiles", TILE_COUNTS)
def test_dead_launch_adds_what_a_live_launch_adds(mtiles):
    live, dead = Device(), Device()
    live.launch("step", mtiles, random.Random(1))
    dead.launch("step", mtiles, random.Random(1), active=False)
    assert live.flags == dead.flags and live.base == dead.base
    dead.launch("step", mtiles, random.Random(2))               # and a live launch behind a dead one finds its targets
    assert all(f == 32 * b for f, b in zip(dead.flags, dead.base))


@pytest.mark.parametrize("seed", range(4))
def test_both_flows_interleaved_with_changing_tile_counts(seed):
    rng = random.Random(50 + seed)
    dev = Device()
    for _ in range(8):
        mtiles = rng.choice(TILE_COUNTS)
        active = rng.random() > 0.2
        if rng.random() < 0.5:
            dev.launch("step", mtiles, rng, active=active)
        else:                                                   # profiling on, or ACEZ_STEP_CHAIN=0: the three-launch flow
            dev.launch("fwd", mtiles, rng, active=active)
            dev.launch("loss_bwd", mtiles, rng, active=active)
        assert all(f == 32 * b for f, b in zip(dev.flags, dev.base))
