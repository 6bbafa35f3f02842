"""CPU: an executable model of the hand-off protocol's progress words (acezero_amd/csrc/head_seq.h:
seq_word, seq_post, seq_poll_expired, seq_catch_up, SEQ_DEAD; head_kernels.hip: rowgemm80_body's post and poll sites, rowseq_loss_stage; head_api.hip:
seq_account). It shares no code with the device.

A row tile owns one 128-byte line of 32 words; word 8 nt + w belongs to wave w of column tile nt (4 workgroups x 8 waves). Seams are
numbered absolutely per row tile: a launch whose base is b completes seams b + 1 .. b + seams(kind). A wave that has finished the stage
in front of seam s stores s into its word (a plain store, one writer per word); the waves that consume seam s read the whole line and
pass when no word is behind s, "behind" being word - s < 0 as a signed 32-bit number.
    layer                 every wave posts its own word; the four loader waves (w >= 4) poll, the multiplier waves follow them
    loss stage            column tile 0: eight waves run two blocks, each posts its own word; column tiles 1..3: waves 0..3 run a block
                          and post their own word AND the word of their loader partner w + 4, waves 4..7 gather and post nothing
    dead launch           one lane per workgroup stores b + seams(kind) into the workgroup's eight words
    fault hook            the launch polls for seam + 2^20 (poll_bias) and posts the true numbers
What is shown: under random wave-level interleavings of the full 32-writer protocol (line reads torn word by word) and under EVERY
interleaving of a reduced one (state-space search), no poll passes before every producer of its seam has finished; a wave that is a
seam ahead lets nobody through early; the loss stage covers all 32 words; a dead launch leaves exactly a live launch's words;
workgroups without a row tile touch nothing; flows, tile counts and dead launches mixed keep words and host bases in step; and all of it
across the wrap of the 32-bit seam number, signed and unsigned."""
import itertools
import random

import pytest

N_FWD, N_BWD = 8, 7
M32 = 0xFFFFFFFF
TILE_COUNTS = [1, 2, 9, 64]
BASES = [0, 5, 2**31 - 7, 2**32 - 7, 2**32 - 1]   # ... + 15 seams: across the signed and the unsigned wrap


def behind(word, target):
    return ((word - target) & M32) >> 31 == 1


def line_passes(line, target):
    return not any(behind(x, target) for x in line)


def decode(block, mtiles):
    per_xcd = (mtiles + 7) >> 3
    jx = block >> 3
    mt = (block & 7) * per_xcd + (jx >> 2)
    return None if mt >= mtiles else (block & 7, mt, jx & 3)


def stages(kind):
    """(name, polls, signals) of the stages a launch runs per row tile; seam i of the launch lies behind its i-th signalling stage."""
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


def runs(name, nt, w):       # does wave w of column tile nt produce anything in this stage?
    return name != "loss" or nt == 0 or w < 4


def polls(name, nt, w):      # ... and does it look at the line before?
    return runs(name, nt, w) if name == "loss" else w >= 4


def waits_for(name, nt, w):  # the waves of its workgroup whose poll stands between this wave and the end of the stage
    if name == "loss":
        return [4 * (w >> 2) + i for i in range(4)] if runs(name, nt, w) else []   # the quartet meets at its LDS counter
    return [4, 5, 6, 7]                                                             # the loader waves' data, through the K loop's barriers


def posted_words(name, nt, w):
    if name != "loss" or nt == 0:
        return [8 * nt + w]
    return [8 * nt + w, 8 * nt + w + 4] if w < 4 else []


class Device:
    def __init__(self, base0=0):
        self.words = [[base0 & M32] * 32 for _ in range(64)]   # (a trainer starts at zero; base0: as if it had run for long)
        self.base = [base0 & M32] * 64
        self.untouched = [True] * 64
        self.partner_writes = 0

    def launch(self, kind, mtiles, rng, active=True, poll_bias=0, budget=None):
        """One launch over `mtiles` row tiles under a random wave-level schedule. Returns the number of polls that expired."""
        st = stages(kind)
        base = list(self.base)                                  # the kernel argument: a snapshot
        for mt in range(mtiles):
            self.base[mt] = (self.base[mt] + seams(kind)) & M32  # seq_account
        wgs = [d for d in map(lambda b: decode(b, mtiles), range(32 * ((mtiles + 7) // 8))) if d]
        assert len(wgs) == 4 * mtiles and len({(mt, nt) for _, mt, nt in wgs}) == 4 * mtiles
        for _, mt, _ in wgs:
            self.untouched[mt] = False
        if not active:                                          # the entry test: one lane per workgroup, eight words
            for _, mt, nt in wgs:
                for w in range(8):
                    self.words[mt][8 * nt + w] = (base[mt] + seams(kind)) & M32
            return 0
        seam_before = [sum(1 for s in st[:i] if s[2]) for i in range(len(st))]
        producers = [{(nt, w) for nt in range(4) for w in range(8) if runs(name, nt, w)} for name, _, _ in st]
        done = {}                                               # (mt, stage) -> the waves that have finished producing it
        # wave: [mt, nt, w, stage, passed its poll, read cursor, polls so far]
        waves = {(mt, nt, w): [mt, nt, w, 0, False, 0, 0] for _, mt, nt in wgs for w in range(8)}
        live = list(waves.values())
        expired = 0
        while live:
            wv = rng.choice(live)
            mt, nt, w, si, passed, cursor, spins = wv
            name, stage_polls, signals = st[si]
            line = self.words[mt]
            if not passed:
                if stage_polls and polls(name, nt, w):
                    target = (base[mt] + seam_before[si] + poll_bias) & M32
                    if behind(line[cursor], target):            # one word of the line at a time: the read may be torn
                        wv[5], wv[6] = 0, spins + 1
                        if budget is not None and wv[6] >= budget:
                            expired += 1
                            wv[4] = True                        # the fault path: goes on with whatever is in memory
                        continue
                    wv[5] = cursor + 1
                    if wv[5] < 32:
                        continue
                    # passed: every producer of the stage in front has finished -- and therefore stored its outputs
                    assert done.get((mt, si - 1), set()) == producers[si - 1], (kind, mt, name, nt, w)
                wv[4] = True
                continue
            mates = [waves[(mt, nt, x)] for x in waits_for(name, nt, w)]
            if any(m[3] < si or (m[3] == si and not m[4]) for m in mates):
                continue                                        # its operands are not there yet
            if runs(name, nt, w):
                done.setdefault((mt, si), set()).add((nt, w))
            if signals:
                value = (base[mt] + seam_before[si] + 1) & M32
                for word in posted_words(name, nt, w):
                    # a word never moves back -- unless a poll has expired: a loader wave of column tiles 1..3 that gave up on the loss
                    # seam may have posted the next one before its partner posts the loss seam for it (the launch's results are
                    # abandoned and the host zeroes every line, seq_fault_check)
                    assert expired or not behind(value, line[word])
                    assert word // 8 == nt                      # ... and stays inside its workgroup's eight
                    self.partner_writes += word != 8 * nt + w
                    line[word] = value
            wv[3], wv[4], wv[5] = si + 1, False, 0
            if wv[3] == len(st):
                live.remove(wv)
        return expired

    def in_step(self, mtiles_seen=64):
        return all(self.words[mt] == [self.base[mt]] * 32 for mt in range(mtiles_seen))


def test_word_layout_and_seam_numbers():
    assert seams("step") == N_FWD + N_BWD == 15 and seams("fwd") + seams("loss_bwd") == 14
    # layers: the 32 waves of a row tile write the 32 words of its line, one each
    assert sorted(x for nt in range(4) for w in range(8) for x in posted_words("fwd0", nt, w)) == list(range(32))
    # the loss stage: 8 + 3 x 4 waves run, and their writes still cover the line exactly once -- the loader partners' words in column
    # tiles 1..3 by the wave four below
    cover = [x for nt in range(4) for w in range(8) if runs("loss", nt, w) for x in posted_words("loss", nt, w)]
    assert sorted(cover) == list(range(32)) and sum(runs("loss", nt, w) for nt in range(4) for w in range(8)) == 20
    for nt in (1, 2, 3):
        for w in range(4):
            assert posted_words("loss", nt, w) == [8 * nt + w, 8 * nt + w + 4] and posted_words("loss", nt, w + 4) == []
    # the poll targets of a launch, in stage order: each seam is polled exactly once, with no factor
    st = stages("step")
    assert [sum(1 for s in st[:i] if s[2]) for i, s in enumerate(st) if s[1]] == list(range(1, 16))


@pytest.mark.parametrize("s", [1, 2**31 - 1, 2**31, 2**32 - 1, 0])
def test_a_wave_that_is_a_seam_ahead_lets_nobody_through(s):
    prev, nxt = (s - 1) & M32, (s + 1) & M32
    assert line_passes([s] * 32, s) and not line_passes([s] * 32, nxt)
    for fast, slow in itertools.permutations(range(0, 32, 5), 2):
        line = [s] * 32
        line[fast] = nxt                     # has already finished the next stage
        assert line_passes(line, s)          # ... which holds nobody up
        assert not line_passes(line, nxt)    # ... and opens nothing: 31 siblings have not finished it
        line[slow] = prev
        assert not line_passes(line, s)      # one sibling behind keeps the seam shut, whatever the others hold
    # a single word at the target is not enough either (the counter form's failure would be a sum that adds up)
    for k in range(32):
        assert not line_passes([prev] * k + [nxt] + [prev] * (31 - k), s)


@pytest.mark.parametrize("base0", BASES)
@pytest.mark.parametrize("mtiles", TILE_COUNTS)
def test_no_poll_passes_before_all_32_producers_and_words_keep_step(mtiles, base0):
    rng = random.Random(mtiles + base0)
    dev = Device(base0)
    for k in range(1, 2 if mtiles == 64 else 4):
        assert dev.launch("step", mtiles, rng) == 0
        assert all(dev.base[mt] == (base0 + 15 * k * (mt < mtiles)) & M32 for mt in range(64)) and dev.in_step()
    assert dev.untouched == [mt >= mtiles for mt in range(64)]   # workgroups without a row tile leave every line alone
    assert dev.partner_writes > 0


@pytest.mark.parametrize("base0", BASES)
@pytest.mark.parametrize("kind", ["step", "fwd", "loss_bwd"])
def test_dead_launch_leaves_a_live_launchs_words(kind, base0):
    for mtiles in (1, 9):
        live, dead = Device(base0), Device(base0)
        live.launch(kind, mtiles, random.Random(1))
        dead.launch(kind, mtiles, random.Random(1), active=False)
        assert live.words == dead.words and live.base == dead.base and dead.in_step()
        assert dead.launch(kind, mtiles, random.Random(2)) == 0    # a live launch behind a dead one finds its seams
        assert dead.in_step()


@pytest.mark.parametrize("seed", range(4))
def test_flows_tile_counts_and_dead_launches_mixed(seed):
    rng = random.Random(50 + seed)
    dev = Device(rng.choice(BASES))
    for _ in range(8):
        mtiles = rng.choice(TILE_COUNTS[:3])
        active = rng.random() > 0.2
        if rng.random() < 0.5:
            dev.launch("step", mtiles, rng, active=active)
        else:                                                   # profiling on, or ACEZ_STEP_CHAIN=0: the three-launch flow
            dev.launch("fwd", mtiles, rng, active=active)
            dev.launch("loss_bwd", mtiles, rng, active=active)
        assert dev.in_step()


@pytest.mark.parametrize("base0", BASES)
def test_the_fault_hooks_seam_never_comes(base0):
    # no word a launch can hold (base .. base + 15) reaches a target moved by 2^20: every poll runs out of its budget, and what the
    # launch posts is untouched by the bias -- the words end where the host's bases are
    for word, seam in itertools.product(range(16), range(1, 16)):
        assert behind((base0 + word) & M32, (base0 + seam + (1 << 20)) & M32)
    dev = Device(base0)
    expired = dev.launch("step", 2, random.Random(3), poll_bias=1 << 20, budget=3)
    assert expired == 2 * (7 * 16 + 20 + 7 * 16) and dev.in_step()   # every polling wave of every seam: layers 4 x 4, the loss stage 20


# ---------------------------------------------------------------------------------------------------
# Every interleaving, by state-space search, of a reduced tile: NT column tiles x W waves (W = 2: one multiplier wave, one loader
# wave that polls; W = 1: the wave polls and posts), three layers = two seams, so that a fast workgroup can be a whole seam ahead of a
# slow one. The state of the line is a function of the waves' progress, so the waves' (stage, passed) pairs are the whole state.
# ---------------------------------------------------------------------------------------------------
def _explore(nt_count, w_count, base0, n_stages=3):
    n = nt_count * w_count
    loader = (lambda w: True) if w_count == 1 else (lambda w: w >= w_count // 2)
    start = tuple((0, True) for _ in range(n))      # stage 0 polls nothing
    seen, stack, passes, finals = {start}, [start], 0, 0
    while stack:
        state = stack.pop()
        # a wave's word: the number of stages it has finished, capped at the signalling ones (the last stage posts nothing)
        line = [(base0 + min(si, n_stages - 1)) & M32 for si, _ in state]
        if all(si == n_stages for si, _ in state):
            finals += 1
            assert line == [(base0 + n_stages - 1) & M32] * n
            continue
        moved = False
        for i, (si, passed) in enumerate(state):
            if si == n_stages:
                continue
            nt, w = divmod(i, w_count)
            nxt = None
            if not passed:
                if not loader(w):
                    nxt = (si, True)
                elif line_passes(line, (base0 + si) & M32):
                    assert all(sj >= si for sj, _ in state), (state, i)   # every writer of the seam has finished the stage in front
                    passes += 1
                    nxt = (si, True)
            else:
                mates = [state[nt * w_count + x] for x in range(w_count) if loader(x)]
                if all(sj > si or (sj == si and pj) for sj, pj in mates):
                    nxt = (si + 1, si + 1 == n_stages)   # (nothing left to poll behind the last stage)
            if nxt is not None:
                moved = True
                new = state[:i] + (nxt,) + state[i + 1:]
                if new not in seen:
                    seen.add(new)
                    stack.append(new)
        assert moved, ("deadlock", state)            # somebody can always move: the protocol cannot hang by itself
    return len(seen), passes, finals


@pytest.mark.parametrize("base0", [0, 2**31 - 2, 2**32 - 2])
@pytest.mark.parametrize("nt_count,w_count", [(4, 1), (2, 2), (3, 2)])
def test_every_interleaving_of_a_reduced_tile(nt_count, w_count, base0):
    states, passes, finals = _explore(nt_count, w_count, base0)
    assert states > 50 and passes > 0 and finals == 1
