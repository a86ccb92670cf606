"""Inputs shared by test_loss_ref.py (CPU) and test_gpu_losses.py (GPU).

Every generator is a pure function of its arguments (own torch.Generator,
CPU tensors), so both suites see the same numbers. Two kinds of input:

* exact-grid: every value is a small multiple of a power of two, so every
  sum the kernels form is exact in fp32 whatever the order, and ties, the
  clip bounds raw == +-1, done rows and w == 0 rows can be planted;
* random-valued: randn-scaled; rows the fp32 kernel may legitimately decide
  differently (top-2 online gap or ||raw| - 1| below EXCL) are reported by
  ``excluded`` and left out of the a*-dependent comparisons.
"""

import math
from types import SimpleNamespace as NS

import torch

GOUT = 0.375           # upstream gradient of every backward
EXCL = 1e-3            # exclusion band of the random-valued cases
EXCL_CAP = 0.05        # at most this share of rows may be excluded
ALPHA = 0.6
# grid cases: gamma^n = 1/4 exactly; random cases: the Ape-X values
GRID_GAMMA, GRID_N = 0.5, 2
RAND_GAMMA, RAND_N = 0.99, 3

DQN_B = (1, 63, 64, 65, 257, 1000)
DQN_A = (2, 6, 18)
QHEAD_B = (1, 3, 4, 5, 31, 33, 130)
# seeds picked from the fp64 reference alone: with them no batch, not even
# B = 1 where one row is everything, loses more than 5 % of its rows to the
# exclusion band, and seed 0 loses none (test_loss_ref.py asserts both)
QHEAD_SEEDS = (0, 3, 5)
HH, QA = 512, 6
# (T, m, n, B, A)
R2D2_SHAPES = ((3, 0, 1, 1, 2), (6, 0, 5, 3, 6), (5, 3, 2, 4, 6),
               (16, 4, 5, 8, 6), (76, 4, 5, 5, 18), (12, 2, 3, 67, 6))
VTRACE_SHAPES = ((1, 1), (1, 65), (20, 32), (80, 300))
VTRACE_CLIPS = ((1.3, 0.7, 0.9), (1.0, 1.0, 1.0))   # rho_bar, c_bar, lam
POLICY_N = (1, 65, 259, 1003)
IMPALA_SHAPES = ((1, 1, 2), (3, 5, 6), (16, 16, 6), (7, 37, 18))  # B, T, A
RESCALE_N = (1, 257, 4099)
SEQPRIO_SHAPES = ((1, 1), (80, 300))
CLIP_N = (1, 3, 4, 5, 1027, 100_003, 2048 * 256 * 8 + 1027)

# unclipped TD errors planted on the grid rows, cycled over the batch:
# the two bounds, just inside (2^-10 off), just outside, well outside, inside
RAW_PLAN = (1.0, -1.0, 1.0 - 2.0 ** -10, -1.0 + 2.0 ** -10, 1.0 + 2.0 ** -10,
            -1.0 - 2.0 ** -10, 2.5, -3.0, 0.25, -0.5, 0.0)


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(hash(tuple(int(k) for k in key)) & 0x7FFFFFFF)
    return g


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _row_plan(B, g):
    """done, w and the planted raw per row. w == 0 on scattered rows and,
    from B = 257 on, on the whole second wave (rows 64..127), so one wave's
    loss contribution is exactly zero."""
    i = torch.arange(B)
    done = (i % 5 == 2).double()
    w = _ints(g, 1, 4, B) / 4.0
    w[i % 7 == 3] = 0.0
    if B >= 257:
        w[64:128] = 0.0
    raw = torch.tensor([RAW_PLAN[k % len(RAW_PLAN)] for k in range(B)],
                       dtype=torch.float64)
    return done, w, raw


# ---------------------------------------------------------------------------
# n-step double-DQN family: q (B, A), or adv (B, A) + val (B,) with dueling
# ---------------------------------------------------------------------------


def dqn_details(q_s, q_on, q_tg, act, rew, done, gamma_n):
    """fp64 a*, raw TD error and top-2 online gap per row."""
    a_star = q_on.argmax(dim=1)
    target = rew + gamma_n * q_tg.gather(1, a_star[:, None])[:, 0] * (1 - done)
    raw = target - q_s.gather(1, act[:, None])[:, 0]
    top2 = q_on.topk(2, dim=1).values
    return a_star, raw, top2[:, 0] - top2[:, 1]


def excluded(raw, gap):
    return (gap < EXCL) | ((raw.abs() - 1.0).abs() < EXCL)


def dqn_grid(B, A, dueling=False):
    """Grid inputs in units of 1/8 (exact in bf16 too). Every third row has
    an exact tie at the top of the online row; the target rows step by 1/2
    per action so a wrong a* moves the target by >= gamma^n / 2 = 1/8.
    With ``dueling`` the three tables are the adv heads: the s and s'
    target rows sum to a multiple of A/8, so the kernel's row mean is exact,
    val is on the grid too and q = adv - mean + val."""
    g = _gen(11, B, A, dueling)
    done, w, raw_want = _row_plan(B, g)
    gamma_n = GRID_GAMMA ** GRID_N
    x_s = _ints(g, -16, 16, B, A)                  # units of 1/8
    x_s[:, 0] += (-x_s.sum(dim=1)) % A             # row sum = 0 mod A
    x_on = _ints(g, -16, 16, B, A)
    tie_lo = torch.full((B,), -1, dtype=torch.long)
    for i in range(0, B, 3):
        j = sorted(torch.randperm(A, generator=g)[:2].tolist())
        x_on[i, j[0]] = x_on[i, j[1]] = 20.0
        tie_lo[i] = j[0]
    perm = torch.stack([torch.randperm(A, generator=g) for _ in range(B)])
    x_tg = perm.double() * 4.0 - 16.0              # row sum = 0 mod A
    q = tuple(x / 8.0 for x in (x_s, x_on, x_tg))
    c = NS(kind="grid", B=B, A=A, gamma=GRID_GAMMA, n_step=GRID_N,
           gamma_n=gamma_n, done=done, w=w, tie_lo=tie_lo, raw_want=raw_want)
    if dueling:
        c.heads = tuple((a, _ints(g, -16, 16, B) / 8.0) for a in q)
        q = tuple(a - a.mean(dim=1, keepdim=True) + v[:, None]
                  for a, v in c.heads)
    c.q = q
    c.act = torch.randint(0, A, (B,), generator=g)
    _, raw0, _ = dqn_details(*q, c.act, torch.zeros(B), done, gamma_n)
    c.rew = raw_want - raw0
    return c


def dqn_random(B, A, seed):
    g = _gen(12, B, A, seed)
    gamma_n = RAND_GAMMA ** RAND_N
    # fp32 values as fp64: the kernel and the reference read the same numbers
    q_s, q_on, q_tg = (torch.randn(B, A, generator=g).double()
                       for _ in range(3))
    act = torch.randint(0, A, (B,), generator=g)
    rew = torch.randn(B, generator=g).double()
    done = (torch.rand(B, generator=g) < 0.2).double()
    w = (torch.rand(B, generator=g) + 0.1).double()
    return NS(kind="random", B=B, A=A, gamma=RAND_GAMMA, n_step=RAND_N,
              gamma_n=gamma_n, act=act, rew=rew, done=done, w=w,
              q=(q_s, q_on, q_tg))


def dueling_random(B, A, seed):
    c = dqn_random(B, A, seed)
    g = _gen(13, B, A, seed)
    heads = []
    for _ in range(3):
        adv = torch.randn(B, A, generator=g).double()
        val = torch.randn(B, generator=g).double()
        heads.append((adv, val))
    c.heads = tuple(heads)
    c.q = tuple(a - a.mean(dim=1, keepdim=True) + v[:, None] for a, v in heads)
    return c


def to_bf16_exact(c):
    """The same case with every Q / head value rounded to bf16 (a no-op on
    the grid), as fp64 again: what a bf16 kernel actually reads."""
    def r(t):
        return t.to(torch.bfloat16).double()

    d = NS(**vars(c))
    if hasattr(c, "heads"):
        d.heads = tuple((r(a), r(v)) for a, v in c.heads)
        d.q = tuple(a - a.mean(dim=1, keepdim=True) + v[:, None]
                    for a, v in d.heads)
    else:
        d.q = tuple(r(q) for q in c.q)
    return d


# ---------------------------------------------------------------------------
# q-head: hidden rows (B, 1024) bf16, heads (6, 512) / (1, 512)
# ---------------------------------------------------------------------------

_TIE_COLS = 8     # tie rows of h_on live on these adv columns only


def _qhead_q(h, wa, ba, wv, bv, pre_act):
    if pre_act:
        h = torch.relu(h)
    adv = h[:, :HH] @ wa.t() + ba
    return adv - adv.mean(dim=1, keepdim=True) + h[:, HH:] @ wv.t() + bv


def _grid_heads(g):
    """wa (6, 512) multiples of 1/64 in [-1/4, 1/4] with wa[j+3] == -wa[j],
    so the adv row sum is sum(ba) = 6/64 and the dueling mean is exact.
    wa[1] == wa[2] == 1/4 and wa[0] == 0 on the first _TIE_COLS columns:
    a hidden row living on those columns ties actions 1 and 2 at the top
    (ba[1] == ba[2])."""
    half = _ints(g, -16, 16, 3, HH) / 64.0
    half[0, :_TIE_COLS] = 0.0
    half[1:, :_TIE_COLS] = 0.25
    wa = torch.cat([half, -half])
    ba = torch.tensor([4, 3, 3, -3, -2, 1], dtype=torch.float64) / 64.0
    wv = _ints(g, -16, 16, 1, HH) / 64.0
    bv = _ints(g, -8, 8, 1) / 64.0
    return wa, ba, wv, bv


def _grid_hidden(g, B, pre_act):
    if pre_act:     # negatives and -0 too: the kernel's ReLU sees them
        h = _ints(g, -3, 3, B, 2 * HH) / 2.0
        h[h == 0] = torch.where(torch.rand(int((h == 0).sum()), generator=g)
                                < 0.5, -0.0, 0.0).double()
        return h
    return _ints(g, 0, 3, B, 2 * HH) / 2.0


def qhead_grid(B, pre_act):
    g = _gen(21, B, pre_act)
    done, w, raw_want = _row_plan(B, g)
    gamma, n_step = GRID_GAMMA, 1           # gamma^n = 1/2
    wa, ba, wv, bv = _grid_heads(g)
    wa_t, ba_t, wv_t, bv_t = _grid_heads(g)
    ba_t = torch.tensor([-15, 9, -9, 15, 3, 3], dtype=torch.float64) / 64.0
    h_s = _grid_hidden(g, B, pre_act)
    h_on = _grid_hidden(g, B, pre_act)
    h_tg = _grid_hidden(g, B, pre_act)
    tie = torch.arange(B) % 3 == 0
    h_on[tie, :HH] = 0.0
    h_on[tie, :_TIE_COLS] = 1.5
    # target rows distinct per action by >= 1/4 (gamma^n / 4 = 1/8 on the
    # target): redraw the rows that are not
    for _ in range(200):
        q_tg = _qhead_q(h_tg, wa_t, ba_t, wv_t, bv_t, pre_act)
        d = (q_tg[:, :, None] - q_tg[:, None, :]).abs()
        d += torch.eye(QA) * 1e9
        bad = d.amin(dim=(1, 2)) < 0.25
        if not bad.any():
            break
        h_tg[bad] = _grid_hidden(g, int(bad.sum()), pre_act)
    act = torch.randint(0, QA, (B,), generator=g)
    q_s = _qhead_q(h_s, wa, ba, wv, bv, pre_act)
    q_on = _qhead_q(h_on, wa, ba, wv, bv, pre_act)
    _, raw0, _ = dqn_details(q_s, q_on, q_tg, act, torch.zeros(B), done,
                             gamma ** n_step)
    rew = raw_want - raw0
    return NS(kind="grid", B=B, pre_act=pre_act, gamma=gamma, n_step=n_step,
              h=(h_s, h_on, h_tg), online=(wa, ba, wv, bv),
              target=(wa_t, ba_t, wv_t, bv_t), act=act, rew=rew, done=done,
              w=w, tie=tie, raw_want=raw_want)


def qhead_random(B, pre_act, seed):
    """randn-scaled and rounded to bf16 (the kernel's input format)."""
    g = _gen(22, B, pre_act, seed)

    def bf(*shape, scale=1.0):
        t = torch.randn(*shape, generator=g) * scale
        return t.to(torch.bfloat16).double()

    def heads():
        return (bf(QA, HH, scale=0.05), bf(QA, scale=0.1),
                bf(1, HH, scale=0.05), bf(1, scale=0.1))

    def hidden():
        h = bf(B, 2 * HH)
        return h if pre_act else torch.relu(h)

    online, target = heads(), heads()
    h = (hidden(), hidden(), hidden())
    act = torch.randint(0, QA, (B,), generator=g)
    rew = torch.randn(B, generator=g).double()
    done = (torch.rand(B, generator=g) < 0.2).double()
    w = (torch.rand(B, generator=g) + 0.1).double()
    return NS(kind="random", B=B, pre_act=pre_act, gamma=RAND_GAMMA,
              n_step=RAND_N, h=h, online=online, target=target, act=act,
              rew=rew.float().double(), done=done, w=w.float().double())


def qhead_ref(c, gout=GOUT, dtype=torch.float64):
    from distributed_rl_amd.ops import torch_ref

    return torch_ref.dueling_q_head_loss_ref(
        c.h[0], *c.online, c.h[1], c.h[2], *c.target, c.act, c.rew, c.done,
        c.w, c.gamma, c.n_step, ALPHA, pre_act=c.pre_act, gout=gout,
        dtype=dtype)


def qhead_excluded(ref):
    top2 = ref["q_on"].topk(2, dim=1).values
    return excluded(ref["raw"], top2[:, 0] - top2[:, 1])


# ---------------------------------------------------------------------------
# R2D2 sequence loss
# ---------------------------------------------------------------------------


def r2d2_case(T, m, n, B, A, seed=0):
    """Values in units of 1/8 (h / h^-1 are not exact, the argmax and the
    identity path are). Online rows tie at the top on every third (t, b);
    done on every other sequence; sequence 0 has td == 0 everywhere when
    rescaling is off (``zero_seq``): its rewards are solved for."""
    g = _gen(31, T, m, n, B, A, seed)
    q_tgt = _ints(g, -16, 16, T, B, A) / 8.0
    q_train = _ints(g, -16, 16, T - m, B, A) / 8.0
    flat = q_train.view(-1, A)
    ties = torch.zeros(flat.shape[0], dtype=torch.bool)
    for i in range(0, flat.shape[0], 3):
        j = torch.randperm(A, generator=g)[:2]
        flat[i, j] = 2.5
        ties[i] = True
    act = torch.randint(0, A, (T, B), generator=g, dtype=torch.int32)
    rew = _ints(g, -8, 8, T, B) / 8.0
    done = (torch.arange(B) % 2 == 0).double()
    w = _ints(g, 1, 4, B) / 4.0
    return NS(T=T, m=m, n=n, B=B, A=A, gamma=0.5, q_train=q_train,
              q_tgt=q_tgt, act=act, rew=rew, done=done, w=w,
              ties=ties.view(T - m, B))


def r2d2_zero_td_case(T, m, n, B, A):
    """The case above with sequence 0 rebuilt so that td == 0 on all of its
    window without rescaling: q_train[ti, 0, a_t] is set to the target,
    walking back from the last window step (a target only looks forward).
    gamma = 1/2 and the 1/8 grid keep every value exact in fp32."""
    from distributed_rl_amd.ops import torch_ref

    c = r2d2_case(T, m, n, B, A, seed=1)
    W = T - 1 - m
    for ti in reversed(range(W)):
        r = torch_ref.r2d2_sequence_loss_ref(
            c.q_train, c.q_tgt, c.act, c.rew, c.done, c.w, m, n, c.gamma,
            0.9, 0.9, False)
        a = int(c.act[m + ti, 0])
        c.q_train[ti, 0, a] += r["td"][ti, 0]
    return c


# ---------------------------------------------------------------------------
# V-trace
# ---------------------------------------------------------------------------


def vtrace_case(T, B, seed=0):
    g = _gen(41, T, B, seed)

    def u(*s):
        return torch.rand(*s, generator=g, dtype=torch.float64)

    b_logp, t_logp = -2.0 * u(T, B), -2.0 * u(T, B)
    rew = torch.randn(T, B, generator=g, dtype=torch.float64)
    val = torch.randn(T, B, generator=g, dtype=torch.float64)
    boot = torch.randn(B, generator=g, dtype=torch.float64)
    not_done = (torch.arange(B) % 4 != 1).double()   # 25 % (B >= 4) done
    if B == 1:
        not_done[:] = 0.0
    f = [t.float().double() for t in (b_logp, t_logp, rew, val, boot)]
    return NS(T=T, B=B, gamma=0.99, b_logp=f[0], t_logp=f[1], rew=f[2],
              val=f[3], boot=f[4], not_done=not_done)


# ---------------------------------------------------------------------------
# IMPALA policy head
# ---------------------------------------------------------------------------


def policy_case(N, A, seed=0):
    """logits * 8; row 0 spreads +-60 so its smallest p underflows in fp32
    (exp(-120) < 1e-38) while log-probabilities stay finite. Actions sit on
    the argmax on even rows and off it on odd rows."""
    g = _gen(51, N, A, seed)
    logits = (torch.randn(N, A, generator=g) * 8.0).double()
    logits[0] = torch.linspace(-60.0, 60.0, A).double()
    am = logits.argmax(dim=1)
    act = torch.where(torch.arange(N) % 2 == 0, am, (am + 1) % A)
    adv = torch.randn(N, generator=g).double()
    return NS(N=N, A=A, logits=logits, act=act, adv=adv)


def impala_case(B, T, A, seed=0):
    """Raw head output (B*(T+1), A+1) with the policy_case logits in the
    t < T rows, plus V-trace targets."""
    g = _gen(52, B, T, A, seed)
    p = policy_case(B * T, A, seed)
    out = (torch.randn(B, T + 1, A + 1, generator=g) * 8.0).double()
    out[:, :T, :A] = p.logits.view(B, T, A)
    out[:, :, A] = torch.randn(B, T + 1, generator=g).double()
    vs = torch.randn(B, T, generator=g).double()
    return NS(B=B, T=T, A=A, out=out.view(B * (T + 1), A + 1), act=p.act,
              adv=p.adv, vs=vs)


def impala_ref(out, act, adv, vs, er, B, T, A, gout=GOUT):
    """fp64 loss / obj / critic / entropy and d(gout * loss)/d out through
    torch_ref.impala_loss on the sliced head output."""
    from distributed_rl_amd.ops import torch_ref

    o = out.detach().clone().requires_grad_(True)
    o3 = o.view(B, T + 1, A + 1)
    logits = o3[:, :T, :A].reshape(B * T, A)
    v = o3[:, :T, A].reshape(B * T)
    total, obj, critic, ent = torch_ref.impala_loss(
        logits, v, act, adv, vs.reshape(-1), er)
    (total * gout).backward()
    return NS(loss=total.detach(), obj=obj.detach(), critic=critic.detach(),
              ent=ent.detach(), dout=o.grad)


# ---------------------------------------------------------------------------
# value rescale, sequence priority, grad clip
# ---------------------------------------------------------------------------


def rescale_grid(n):
    """+-{0, -0, logspace 1e-6 .. 1e4} cycled to n values."""
    mags = torch.logspace(-6, 4, 41, dtype=torch.float64)
    base = torch.cat([torch.tensor([0.0, -0.0], dtype=torch.float64), mags,
                      -mags]).float().double()
    return base[torch.arange(n) % base.numel()].clone()


def seqprio_case(T, B):
    """|td| (T, B): column 0 all zero, column 1 (if any) max at t = 0,
    column 2 max at t = T-1."""
    g = _gen(61, T, B)
    td = torch.rand(T, B, generator=g).double()
    td[:, 0] = 0.0
    if B > 2:
        td[0, 1] = 3.0
        td[T - 1, 2] = 3.0
    return td


def clip_case(n, seed=0):
    g = _gen(71, n, seed)
    return torch.randn(n, generator=g) * 3.0      # fp32: the kernel's input


def band_shares(c, rho_bar, c_bar):
    rho = (c.t_logp - c.b_logp).exp()
    n = rho.numel()
    return (float((rho > rho_bar).sum()) / n, float((rho < c_bar).sum()) / n,
            float(((rho >= c_bar) & (rho <= rho_bar)).sum()) / n)


def ulp_bf16(ref):
    """Half a bf16 ulp of the reference, per element: bf16 keeps 8
    significant bits, so for 2^e <= |ref| < 2^(e+1) the ulp is 2^(e-7) and
    round-to-nearest is off by up to 2^(e-8). That is between 2^-9 |ref|
    (just below a power of two) and 2^-8 |ref| (at one); the blanket
    2^-9 |ref| would fail a correctly rounding kernel."""
    mant, exp = torch.frexp(ref.abs())          # |ref| = mant * 2^exp, mant in [.5, 1)
    half = torch.ldexp(torch.ones_like(mant), exp - 9)
    return torch.where(ref == 0, torch.zeros_like(half), half)


def rel_err(got, ref, floor):
    """max |got - ref| / max(|ref|, floor), in fp64."""
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().reshape(-1)
    assert got.shape == ref.shape
    if got.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / ref.abs().clamp_min(floor)).max())


assert math.isclose(GRID_GAMMA ** GRID_N, 0.25)
