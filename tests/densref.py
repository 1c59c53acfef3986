"""Plain numpy restatements shared by the per-Gaussian score and mixture-selection tests.

dens_ref() is compute_g_base() (libsent/src/phmm/gprune_none.c:59-82) in fp32 with the operation order of
gmm_dens_kernel: acc = gconst; per dimension x = o - mu; x = x * x; x = x * ivar; acc = acc + x; then acc * -0.5,
every step rounded to float32.  A NULL density gives LOG_ZERO.  gmax_winners() is the visiting order of
compute_g_max() (libsent/src/phmm/gms_gprune.c:132-178) over such scores; the other helpers turn its winners into
the conditions the selection tests assert about their own inputs."""
import numpy as np

LOG_ZERO = np.float32(-1000000.0)
INV_LOG_TEN = .434294482                                     # libsent/include/sent/stddefs.h:111, a double


def dens_columns(model):
    """Density index of every score column (-1: NULL density) and the codebook offsets (None for a plain model).
    A plain model's columns are its mixture entries in state order; an all-tied-mixture model's are its codebook
    Gaussians, book after book: column book_offsets[b] + k is Gaussian k of codebook b, read from the first state
    tied to b (GCODEBOOK.d[], htk_hmm.h:196-201)."""
    ent_dens, st_off = np.asarray(model["ent_dens"]), np.asarray(model["st_off"])
    st_book = model.get("st_book")
    if st_book is None or int(model.get("nbook", 0)) == 0:
        return ent_dens.astype(np.int64), None
    st_book = np.asarray(st_book)
    assert (st_book >= 0).all(), "no single column order for a model that mixes plain and tied states"
    cols, off = [], [0]
    for b in range(int(model["nbook"])):
        s = int(np.nonzero(st_book == b)[0][0])
        cols.append(ent_dens[st_off[s]:st_off[s + 1]])
        off.append(off[-1] + len(cols[-1]))
    return np.concatenate(cols).astype(np.int64), np.array(off, np.int32)


def dens_ref(model, frames):
    """[T][ncolumn] float32 per-Gaussian scores in the column order of dens_columns()."""
    dens, _ = dens_columns(model)
    g = np.maximum(dens, 0)
    fr = np.asarray(frames, dtype=np.float32)
    mean, ivar = np.asarray(model["mean"], np.float32), np.asarray(model["ivar"], np.float32)
    acc = np.broadcast_to(np.asarray(model["gconst"], np.float32)[g][None, :], (len(fr), len(g))).astype(np.float32)
    with np.errstate(over="ignore"):
        for d in range(fr.shape[1]):
            x = (fr[:, None, d] - mean[g, d][None, :]).astype(np.float32)
            x = (x * x).astype(np.float32)
            x = (x * ivar[g, d][None, :]).astype(np.float32)
            acc = (acc + x).astype(np.float32)
        out = (acc * np.float32(-0.5)).astype(np.float32)
    out[:, dens < 0] = LOG_ZERO
    return out


def gmax_winners(st_off, dens, utt_off=None):
    """compute_g_max() with LAST_BEST over dens [T][E]: the previous frame's winner of the state is scored first
    (the last entry on an utterance's first frame) and floored at LOG_ZERO, then the entries n-1 .. 0 without it
    under a strict >.  Hence the winner is the HIGHEST index among the entries that share the maximum when that
    maximum beats the first one, and the first one otherwise.  Returns (win [T][S] int, maxprob [T][S] float32)."""
    st_off = np.asarray(st_off)
    T, S = len(dens), len(st_off) - 1
    utt_off = [0, T] if utt_off is None else list(utt_off)
    win, mp = np.zeros((T, S), np.int64), np.zeros((T, S), np.float32)
    for a, b in zip(utt_off[:-1], utt_off[1:]):
        for i in range(S):
            e0, n = int(st_off[i]), int(st_off[i + 1] - st_off[i])
            last = -1
            for t in range(a, b):
                v = dens[t, e0:e0 + n]
                first = last if last != -1 else n - 1
                best, maxi = max(v[first], LOG_ZERO), first
                m = v.max()
                if m > best:
                    best, maxi = m, n - 1 - int(np.argmax(v[::-1]))
                win[t, i], mp[t, i], last = maxi, best, maxi
    return win, mp


def visiting_order_covered(st_off, win, utt_off=None):
    """What the winners say about the four-wide loop of gms_select_kernel (k = n-1, n-5, ... in groups of four, then a
    scalar tail of n % 4 entries).  Returns (residues, changed, in_body, in_tail): the largest set of classes
    (n - 1 - k) % 4 that the winners k of ONE state fall in, whether some winner differs from the previous frame's
    winner of its utterance, whether a winner lay in a four-wide group and whether one lay in the scalar tail."""
    st_off = np.asarray(st_off)
    n = np.diff(st_off)
    T = len(win)
    utt_off = [0, T] if utt_off is None else list(utt_off)
    res = (n[None, :] - 1 - win) % 4
    residues = max((set(int(r) for r in np.unique(res[:, i])) for i in range(len(n))), key=len)
    changed = any((win[a + 1:b] != win[a:b - 1]).any() for a, b in zip(utt_off[:-1], utt_off[1:]) if b - a > 1)
    tail = n % 4                                              # entries 0 .. tail-1 are left to the scalar loop
    in_tail = bool((win < tail[None, :]).any())
    in_body = bool((win >= tail[None, :]).any())              # (with n < 4 the tail is the whole state)
    return residues, changed, in_body, in_tail


def gms_state_scores(model, dens, utt_off=None, win=None):
    """The selection states' scores of every frame, compute_g_max()'s return value: the winner's score plus the
    weight of the winner (or of `win` [T][S] where given), a float32 sum, times INV_LOG_TEN in double."""
    st_off, logw = np.asarray(model["st_off"]), np.asarray(model["ent_logw"], np.float32)
    w, mp = gmax_winners(st_off, dens, utt_off)
    if win is not None:
        w = win
    s = (mp + logw[st_off[:-1][None, :] + w]).astype(np.float32)
    return (s.astype(np.float64) * INV_LOG_TEN).astype(np.float32)


def boundary_is_untied(fs, nbest):
    """No frame on which the nbest-th and the next selection state score the same: only then is the selected set
    independent of the order in which ties fall, and the ranking form bound to the reference's choice."""
    if nbest >= fs.shape[1]:
        return True
    srt = -np.sort(-fs, axis=1)
    return bool((srt[:, nbest - 1] != srt[:, nbest]).all())
