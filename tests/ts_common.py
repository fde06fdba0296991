"""lsdr_ts_batch's definition (include/lsdr_hip.h) restated in numpy — a test oracle, never imported by the product — and a builder of
transport streams with a known list of injected events.

census(ts, max_pids) returns what capi.TsBatch.census returns for one stream: the summary dict with "pids": [dict per listed PID].
kept(ts, …) is the filter's selection: the indices of the packets a rule keeps.
"""
import numpy as np

NULL_PID = 0x1fff
PCR_MOD = (1 << 33) * 300


def packets_of(ts):
    a = np.frombuffer(ts, np.uint8) if isinstance(ts, (bytes, bytearray)) else np.ascontiguousarray(ts, np.uint8).reshape(-1)
    assert len(a) % 188 == 0
    return a.reshape(-1, 188)


def fields(ts):
    """Every packet's class (0 valid, 1 bad sync byte, 2 TEI) and, for the valid ones, its fields."""
    b = packets_of(ts).astype(np.int64)
    cls = np.where(b[:, 0] != 0x47, 1, np.where(b[:, 1] & 0x80, 2, 0))
    afc = (b[:, 3] >> 4) & 3
    af = afc >> 1
    af_len = np.where(af == 1, b[:, 4], 0)
    base = (b[:, 6] << 25) | (b[:, 7] << 17) | (b[:, 8] << 9) | (b[:, 9] << 1) | (b[:, 10] >> 7)
    ext = ((b[:, 10] & 1) << 8) | b[:, 11]
    return dict(cls=cls, pid=((b[:, 1] & 0x1f) << 8) | b[:, 2], pusi=(b[:, 1] >> 6) & 1, scrambled=((b[:, 3] & 0xc0) != 0).astype(np.int64),
                payload=afc & 1, cc=b[:, 3] & 15, disc=((af == 1) & (af_len > 0) & ((b[:, 5] & 0x80) != 0)).astype(np.int64),
                pcr=((af == 1) & (af_len >= 7) & ((b[:, 5] & 0x10) != 0)).astype(np.int64), pcr_value=base * 300 + ext)


def census(ts, max_pids=64):
    f = fields(ts)
    n = len(f["cls"])
    valid = np.flatnonzero(f["cls"] == 0)
    pid = f["pid"][valid]
    order = valid[np.argsort(pid, kind="stable")]                         # by PID, stream order inside a PID
    p_sorted = f["pid"][order]
    # the pair rule on consecutive packets of one PID
    prev, cur = order[:-1], order[1:]
    pair = (p_sorted[:-1] == p_sorted[1:]) & (p_sorted[1:] != NULL_PID)
    prev, cur = prev[pair], cur[pair]
    disc = f["disc"][cur] == 1
    expected = (f["cc"][prev] + f["payload"][cur]) & 15
    fine = f["cc"][cur] == expected
    repeat = ~disc & ~fine & (f["payload"][cur] == 1) & (f["cc"][cur] == f["cc"][prev])
    error = ~disc & ~fine & ~repeat
    missing = np.where(error, (f["cc"][cur] - expected) & 15, 0)
    cur_pid = f["pid"][cur]

    def per_pid(index, weights):
        out = np.zeros(8192, np.int64)
        np.add.at(out, index, weights)
        return out
    packets = per_pid(pid, np.ones(len(valid), np.int64))
    c = dict(packets=packets, pusi=per_pid(pid, f["pusi"][valid]), scrambled=per_pid(pid, f["scrambled"][valid]), pcr_count=per_pid(pid, f["pcr"][valid]),
             cc_errors=per_pid(cur_pid, error.astype(np.int64)), cc_repeats=per_pid(cur_pid, repeat.astype(np.int64)),
             cc_missing=per_pid(cur_pid, missing), discontinuities=per_pid(cur_pid, disc.astype(np.int64)))
    seen = np.flatnonzero(packets)
    table = []
    for p in seen[:max_pids]:
        idx = valid[pid == p]
        r = dict(pid=int(p), first_packet=int(idx[0]), last_packet=int(idx[-1]))
        r.update({k: int(v[p]) & 0xffffffff for k, v in c.items()})
        table.append(r)
    s = dict(packets=n, sync_errors=int((f["cls"] == 1).sum()), tei=int((f["cls"] == 2).sum()), null_packets=int(packets[NULL_PID]),
             valid=len(valid), cc_errors=int(c["cc_errors"].sum()), cc_repeats=int(c["cc_repeats"].sum()), cc_missing=int(c["cc_missing"].sum()),
             discontinuities=int(c["discontinuities"].sum()), kept=0, pcr_first=0, pcr_last=0, pcr_first_packet=0, pcr_last_packet=0,
             pids_seen=len(seen), pids_listed=min(len(seen), max_pids), pcr_pid=-1, pcr_count=0)
    with_pcr = valid[f["pcr"][valid] == 1]
    if len(with_pcr):
        p = int(f["pid"][with_pcr[0]])
        mine = with_pcr[f["pid"][with_pcr] == p]
        s.update(pcr_pid=p, pcr_count=len(mine), pcr_first_packet=int(mine[0]), pcr_last_packet=int(mine[-1]),
                 pcr_first=int(f["pcr_value"][mine[0]]), pcr_last=int(f["pcr_value"][mine[-1]]))
    s["pids"] = table
    return s


def kept(ts, keep_pids=None, drop_null=True, drop_tei=True, drop_sync=True):
    """The indices of the packets the rule keeps, ascending."""
    f = fields(ts)
    cls, pid = f["cls"], f["pid"]
    listed = np.ones(len(cls), bool) if keep_pids is None else np.isin(pid, np.asarray(list(keep_pids), np.int64))
    keep = np.where(cls == 1, not drop_sync, np.where(cls == 2, not drop_tei, listed & ~((pid == NULL_PID) & bool(drop_null))))
    return np.flatnonzero(keep)


def select(ts, idx):
    return packets_of(ts)[idx].tobytes()


# ---- the builder -------------------------------------------------------------------------------------------------------------------
PAT, VIDEO, AUDIO, DATA = 0x0000, 0x0100, 0x0101, 0x0102
TICKS_PER_PACKET = 4000                                                   # 27 MHz ticks: 188·8·27e6/4000 = 10.152 Mbit/s


def pcr_bytes(value):
    base, ext = value // 300, value % 300
    return [base >> 25, (base >> 17) & 255, (base >> 9) & 255, (base >> 1) & 255, ((base & 1) << 7) | 0x7e | (ext >> 8), ext & 255]


def build_stream(n=3000, seed=7, events=True):
    """A TS of about n packets on five PIDs — PAT, video (58 %, a PCR on every 25th of its packets, the 33-bit base wrapping in the middle
    of the stream), audio (some packets scrambled), data (three in ten of its packets carry an adaptation field only) and 20 % null
    packets with arbitrary counters — with correct continuity counters, and then (events), far from one another:
      a legal duplicate and a triple repeat on video (cc_repeats 1 + 2), a discontinuity flag with a counter jump on audio, a TEI bit on
      one audio payload packet (its successor: one error, missing 1) and on two null packets, a bad sync byte on a null packet, three
      consecutive video payload packets deleted (one error, missing 3), one data payload packet deleted (one error, missing 1) and one
      data packet with an adaptation field only deleted (no trace: cc_missing is a lower bound).
    Returns (the packets as uint8 [N][188], the expected figures: totals and per PID)."""
    rng = np.random.default_rng(seed)
    pid_of = [PAT, VIDEO, AUDIO, DATA, NULL_PID]
    kinds = rng.choice(5, n, p=[0.02, 0.58, 0.12, 0.08, 0.20])
    cc = {p: int(rng.integers(0, 16)) for p in pid_of}
    pk = rng.integers(0, 256, (n, 188)).astype(np.uint8)
    meta = []
    videos = 0
    for k in range(n):
        pid = pid_of[kinds[k]]
        afc, pusi, scr, pcr = 1, 0, 0, False
        if pid == DATA and rng.random() < 0.3:
            afc = 2
        if pid == VIDEO:
            videos += 1
            pusi = int(videos % 10 == 0)
            if videos % 25 == 1:
                afc, pcr = 3, True
        if pid == PAT:
            pusi = 1
        if pid == AUDIO and rng.random() < 0.25:
            scr = 2
        if pid == NULL_PID:
            cc[pid] = int(rng.integers(0, 16))                            # never checked
        else:
            cc[pid] = (cc[pid] + (afc & 1)) & 15
        pk[k, 0], pk[k, 1], pk[k, 2], pk[k, 3] = 0x47, (pusi << 6) | (pid >> 8), pid & 255, (scr << 6) | (afc << 4) | cc[pid]
        if afc == 2:
            pk[k, 4], pk[k, 5] = 183, 0
        if pcr:
            pk[k, 4], pk[k, 5] = 7, 0x10
        meta.append(dict(pid=pid, afc=afc, pcr=pcr))

    rows = list(range(n))                                                 # the source row of every packet of the result
    if events:
        def first_after(frac, ok):
            for k in range(int(frac * n), n):
                if ok(k):
                    return k
            raise AssertionError("the stream is too short for its events")

        def has_successor(k):
            return any(m["pid"] == meta[k]["pid"] for m in meta[k + 1:])

        plain = lambda pid: (lambda k: meta[k]["pid"] == pid and meta[k]["afc"] == 1 and has_successor(k))
        # in place
        k = first_after(0.35, plain(AUDIO))
        pk[k, 3] = (pk[k, 3] & 0xcf) | 0x30
        pk[k, 4], pk[k, 5] = 1, 0x80
        for j in range(k, n):
            if meta[j]["pid"] == AUDIO:
                pk[j, 3] = (pk[j, 3] & 0xf0) | ((pk[j, 3] + 5) & 15)
        k = first_after(0.45, plain(AUDIO))
        pk[k, 1] |= 0x80
        for frac in (0.50, 0.52):
            k = first_after(frac, lambda k: meta[k]["pid"] == NULL_PID and not pk[k, 1] & 0x80)
            pk[k, 1] |= 0x80
        k = first_after(0.55, lambda k: meta[k]["pid"] == NULL_PID and not pk[k, 1] & 0x80)
        pk[k, 0] = 0x46
        # insertions and deletions, the last first

        def three_videos(k):
            v = [j for j in range(k, n) if meta[j]["pid"] == VIDEO][:4]
            return meta[k]["pid"] == VIDEO and len(v) == 4 and all(meta[j]["afc"] == 1 for j in v[:3])
        k = first_after(0.85, lambda k: meta[k]["pid"] == DATA and meta[k]["afc"] == 2 and has_successor(k))
        del rows[k]
        k = first_after(0.75, plain(DATA))
        del rows[k]
        k = first_after(0.65, three_videos)
        for j in [j for j in range(k, n) if meta[j]["pid"] == VIDEO][:3][::-1]:
            del rows[j]
        k = first_after(0.25, plain(VIDEO))
        rows[k:k] = [k, k]
        k = first_after(0.15, plain(VIDEO))
        rows[k:k] = [k]
    out = pk[rows].copy()
    # the PCRs from the final places: the base wraps in the middle
    start = PCR_MOD - TICKS_PER_PACKET * (len(out) // 2) - 123
    for k, r in enumerate(rows):
        if meta[r]["pcr"]:
            out[k, 6:12] = pcr_bytes((start + TICKS_PER_PACKET * k) % PCR_MOD)
    if not events:
        none = dict(cc_errors=0, cc_missing=0, cc_repeats=0, discontinuities=0)
        return out, dict(packets=n, sync_errors=0, tei=0, pcr_pid=VIDEO, per_pid={p: dict(none) for p in pid_of}, **none)
    expected = dict(packets=len(out), sync_errors=1, tei=3, cc_errors=3, cc_missing=5, cc_repeats=3, discontinuities=1, pcr_pid=VIDEO,
                    per_pid={PAT: dict(cc_errors=0, cc_missing=0, cc_repeats=0, discontinuities=0),
                             VIDEO: dict(cc_errors=1, cc_missing=3, cc_repeats=3, discontinuities=0),
                             AUDIO: dict(cc_errors=1, cc_missing=1, cc_repeats=0, discontinuities=1),
                             DATA: dict(cc_errors=1, cc_missing=1, cc_repeats=0, discontinuities=0),
                             NULL_PID: dict(cc_errors=0, cc_missing=0, cc_repeats=0, discontinuities=0)})
    return out, expected
