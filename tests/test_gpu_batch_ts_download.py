"""The TS download of the batch decoders (lsdr_capture_batch_ts_download_async / lsdr_hs_batch_ts_download_async and their _ts_wait): one
implementation in the FEC tail (tail_host.h) behind the default engine, the Viterbi engine and lsdr_hs_batch.

A download that is still pending when the next batch is queued delivers the batch it was asked for: the tail makes the kernel that
writes the TS buffers wait for it.  Refused: a download before the first wait, and one into host buffers a byte too small.
"""
import ctypes as C

import pytest
from batch_common import capture

pytestmark = pytest.mark.gpu

N = 300000          # 250 000 symbols: about 150 packets sent, more than 50 decoded (test_gpu_hs_batch's short run)


def _object(capi, ctx, engine):
    if engine == "hs":
        return capi.HsBatch(ctx, 2, N, 1.2)
    return capi.CaptureBatch(ctx, 2, N, 1.2, anf=0, tile_len=4096, tile_warmup=512, viterbi=engine == "viterbi")


@pytest.mark.parametrize("engine", ["default", "viterbi", "hs"])
def test_a_pending_download_delivers_its_own_batch(capi, ctx, engine):
    # two 600-packet captures carry the same packets (the seed is the noise's), so the second one is cut from the middle of its capture: a batch
    # with the two swapped then has another TS in every host buffer
    bufs = [ctx.upload(capture(600, seed, noise)[0][2 * first: 2 * (first + N)]) for seed, noise, first in ((21, 6.0, 0), (24, 7.5, 600000))]
    a, b = [bufs[0].ptr, bufs[1].ptr], [bufs[1].ptr, bufs[0].ptr]
    obj = _object(capi, ctx, engine)
    host = [C.c_void_p(), C.c_void_p()]
    try:
        obj.run_async(a, N)
        with pytest.raises(capi.LsdrError):                   # before the first wait
            obj.ts_download_async(host, 0)
        obj.wait()
        res_a, ts_a = obj.decode(a, N)
        print(f"{engine}: packets {[r['ts_packets'] for r in res_a]}")
        # condition on the input: both captures decode, to different TS
        assert all(len(t) >= 50 * 188 for t in ts_a) and ts_a[0] != ts_a[1], [len(t) for t in ts_a]
        need = max(len(t) for t in ts_a)
        for h in host:
            capi.check(capi.lib.lsdr_malloc_host(need, C.byref(h)))
            C.memset(h, 0xEE, need)

        def got(i, n):
            return C.string_at(host[i], n)

        obj.run_async(a, N)
        assert obj.wait() == res_a
        with pytest.raises(capi.LsdrError):
            obj.ts_download_async(host, need - 1)
        obj.ts_download_async(host, need)
        obj.run_async(b, N)                                   # the download may still be under way
        obj.ts_wait()
        res_b = obj.wait()
        assert [got(i, len(ts_a[i])) for i in range(2)] == ts_a, "the pending download did not deliver the batch it was asked for"
        assert res_b == res_a[::-1]
        obj.ts_download_async(host, need)
        obj.ts_wait()
        assert [got(i, len(ts_a[1 - i])) for i in range(2)] == ts_a[::-1], "the following download is not the second batch's TS"
    finally:
        obj.close()
        for h in host:
            if h.value:
                capi.lib.lsdr_free_host(h)
        for d in bufs:
            d.free()
