// leansdr_amd/csrc/tail_relock.h — the window and rewind arithmetic of the FEC tail's re-acquisition (tail_device.h: k_tail_relock).
// Plain integer functions, __host__ __device__: the kernel uses them, and tests/tail_relock_host.hip checks them on the host against a
// loop of single windows.
//
// With re-acquisition on, a capture's deconvolver is never more than one `window`-byte pipe ahead of mpeg_sync — the schedule of the
// reference's graph.  While mpeg_sync is locked the device still deconvolves a whole stretch in one launch; that is exact because
//   · K consecutive calls of deconvol_sync::run with `window` bytes of room each (dvb.h:419-470) write the bytes of ONE call with
//     K·window bytes of room and leave the same counters, as long as every one of the K calls is a whole window (relock_whole_windows),
//   · mpeg_sync's locked path takes whole packets with one byte of look-ahead (dvb.h:842-846): where the lock drops at packet `drop_at`
//     of the stretch, the windowed schedule notices it in the first window whose end covers that packet and the look-ahead byte
//     (relock_drop_windows) — the bytes up to that window's end stand, the deconvolver is put back there (relock_call over the kept
//     windows, relock_after) and the window loop goes on from that boundary.
#ifndef LSDR_TAIL_RELOCK_H
#define LSDR_TAIL_RELOCK_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RELOCK_HD __host__ __device__
#else
#define RELOCK_HD
#endif

constexpr unsigned long long kRelockPacket = 204;      // mpeg_sync's packets in front of the deinterleaver (RS(204,188))
constexpr unsigned kRelockMax = 16;                    // most re-acquisitions an object can be asked for

// deconvol_sync at the alignment in force: symbols consumed, bytes written, bits in the shift register, bits pending (dvb.h:297-306)
struct relock_dec { unsigned long long pos, bw; int n_in, n_out; };
// one call's sizes: bytes written, refills, symbols consumed, symbols of refill 0, bits pending afterwards
struct relock_call { unsigned long long n, refills, used; unsigned m0; int n_out_end; };

// deconvol_sync::run's sizes for one call with `cap` bytes of room (dvb.h:419-470; in.read(skip) already done): n = 0 — nothing moves
RELOCK_HD inline relock_call relock_plan_call(int pp, int pw, unsigned long long nsym, const relock_dec &s, unsigned long long cap) {
  relock_call c = {0, 0, 0, 0, s.n_out};
  const unsigned long long readable = nsym > s.pos ? nsym - s.pos : 0;
  if (readable < 64) return c;
  const long long maxrd = (long long)((readable - 64) / (unsigned)(pw / 2) * (unsigned)pp / 8);
  const long long n = maxrd < (long long)cap ? maxrd : (long long)cap;
  if (n < 32) return c;
  const long long need = 8 * n - s.n_out;
  const unsigned long long R = need > 0 ? (unsigned long long)((need + pp - 1) / pp) : 0;
  c.m0 = s.n_in < 64 ? (unsigned)((64 - s.n_in + 1) / 2) : 0u;
  c.n = (unsigned long long)n;
  c.refills = R;
  c.n_out_end = (int)(s.n_out + (long long)R * pp - 8 * n);
  c.used = R ? c.m0 + (R - 1) * (unsigned)(pw / 2) : 0;
  return c;
}
// … and the counters behind it
RELOCK_HD inline relock_dec relock_after(int pw, relock_dec s, const relock_call &c) {
  if (c.refills) s.n_in = 64 - pw;
  s.n_out = c.n_out_end;
  s.pos += c.used;
  s.bw += c.n;
  return s;
}

// window j (0, 1, …) behind s is a WHOLE one — its call writes exactly `window` bytes — given that the windows in front of it are
RELOCK_HD inline bool relock_window_whole(int pp, int pw, unsigned long long nsym, unsigned long long byte_cap, unsigned long long window,
                                          const relock_dec &s, unsigned long long j) {
  if (byte_cap < s.bw || (byte_cap - s.bw) / window < j + 1) return false;
  relock_dec t = s;
  if (j) {                                             // the counters behind j whole windows: one call of j·window bytes
    const long long need = 8 * (long long)(j * window) - s.n_out;
    const unsigned long long R = (unsigned long long)((need + pp - 1) / pp);
    const unsigned m0 = s.n_in < 64 ? (unsigned)((64 - s.n_in + 1) / 2) : 0u;
    const unsigned long long used = m0 + (R - 1) * (unsigned)(pw / 2);
    if (nsym < s.pos || used > nsym - s.pos) return false;
    t.pos = s.pos + used; t.bw = s.bw + j * window; t.n_in = 64 - pw; t.n_out = (int)(s.n_out + (long long)R * pp - 8 * (long long)(j * window));
  }
  return relock_plan_call(pp, pw, nsym, t, window).n == window;
}

// The split of a locked stretch: how many whole windows behind s ONE call of K·window bytes stands for (the rest of the stream — less
// than a window here, or a call that the symbols or the room cut short — is walked window by window).  Largest K with windows
// 0 … K−1 whole and the one call itself not cut short by its own size rule.
RELOCK_HD inline unsigned long long relock_whole_windows(int pp, int pw, unsigned long long nsym, unsigned long long byte_cap, unsigned long long window,
                                                         const relock_dec &s) {
  if (byte_cap < s.bw) return 0;
  unsigned long long hi = (byte_cap - s.bw) / window;                    // K ≤ hi
  {
    const unsigned long long one = relock_plan_call(pp, pw, nsym, s, hi * window).n / window;
    if (one < hi) hi = one;
  }
  unsigned long long lo = 0;                                             // windows 0 … lo−1 are whole (whole-ness is monotone in j)
  while (lo < hi) {
    const unsigned long long mid = lo + (hi - lo + 1) / 2;
    if (relock_window_whole(pp, pw, nsym, byte_cap, window, s, mid - 1)) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The lock drops at packet drop_at (0, 1, …) of a locked stretch that began with `lead` bytes deconvolved but not yet taken by mpeg_sync
// (lead ≤ 204: mpeg_sync had run until nothing moved).  Returns how many of the stretch's windows stand: the drop is noticed in the
// first window whose end covers the packet and one byte of look-ahead.
RELOCK_HD inline unsigned long long relock_drop_windows(unsigned long long drop_at, unsigned long long lead, unsigned long long window) {
  const unsigned long long want = (drop_at + 1) * kRelockPacket + 1;      // bytes behind the stretch's first unread byte
  if (want <= lead) return 1;
  return (want - lead + window - 1) / window;
}

#endif  // LSDR_TAIL_RELOCK_H
