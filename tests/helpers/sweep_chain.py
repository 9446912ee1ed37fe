"""The chain of existing public calls that ``sweep_batch()`` must equal bit for bit, written once from public objects, and the
scenes of the sweep tests.

    simulate_batch -> mix.astype(float32) -> BatchSTFT.analysis_device -> the plan calls of the solver, with the same chunks of
    iterate() -> demix_device -> synthesis_device -> order = argsort(-std, stable) -> y[:m] and ref[:K + 1, :m, ref_mic] ->
    bss_eval_batch

The ordering is only as good as the gap between the standard deviations: ``evaluate`` asserts, on the chain's own values, that
neighbouring sorted standard deviations differ by more than ``MIN_GAP`` relative wherever an ordering is taken.

Scenes: fs 8000, image order 2, 4 sources (2 targets) and 3 microphones, frame 64 and hop 32, 16 filter taps, three rooms that
differ in size, geometry and absorption.  "dense": one signal length and one impulse response length; "ragged": three signal
lengths and ``rir_length=None``."""
import functools

import numpy as np

import room_cases as cases

MIN_GAP = 1e-9
FS, ORDER, S, M, K = 8000, 2, 4, 3, 2
FRAME, HOP, LF = 64, 32, 16
ROOMS = (
    dict(room_dim=cases.SMALL, absorption=0.3, seed=41),
    dict(room_dim=cases.MID, absorption=0.2, seed=42),
    dict(room_dim=(4.0, 6.0, 3.1), absorption=0.5, seed=43),
)
LENGTHS = {"dense": (2400, 2400, 2400), "ragged": (2000, 2500, 3000)}
RIR_LENGTH = {"dense": 300, "ragged": None}
SOURCES_VAR = (1.0, 0.5)
SINR, SNR, REF_MIC = 5.0, 30.0, 1


@functools.lru_cache(maxsize=None)
def scene(kind, n_targets=K):
    """-> the keyword arguments of ``sweep_batch`` for the three rooms (signals a list for "ragged"), read-only"""
    geo = [cases.geometry(r["room_dim"], S, M, r["seed"]) for r in ROOMS]
    rng = np.random.default_rng(7)
    signals = [rng.standard_normal((S, n)) * np.repeat(rng.gamma(2.0, 1.0, (S, n // 200 + 1)), 200, axis=1)[:, :n]
               for n in LENGTHS[kind]]
    longest = max(LENGTHS[kind]) + 2000
    noise = [rng.standard_normal((longest, M)) for _ in ROOMS]       # cut to n_out once the lengths are known
    filler = [rng.standard_normal(longest) for _ in ROOMS]
    var = SOURCES_VAR[:n_targets]
    return dict(signals=signals if kind == "ragged" else np.stack(signals), room_dim=np.array([r["room_dim"] for r in ROOMS], float),
                sources=np.stack([g[0] for g in geo]), mics=np.stack([g[1] for g in geo]),
                absorption=np.array([r["absorption"] for r in ROOMS]), fs=FS, max_order=ORDER, rir_length=RIR_LENGTH[kind],
                n_targets=n_targets, sinr=SINR, snr=SNR, ref_mic=REF_MIC, sources_var=var, frame=FRAME, hop=HOP, filter_length=LF,
                filler=filler, _noise=noise)


def pick(args, rooms):
    """the arguments of some rooms of a scene"""
    out = dict(args)
    for key in ("signals", "room_dim", "sources", "mics", "absorption", "filler", "_noise"):
        v = [args[key][b] for b in rooms]
        out[key] = v if isinstance(args[key], list) else np.stack(v)
    return out


def with_noise(args, out_lengths):
    """the scene with its noise cut to the rooms' output lengths, in the form ``signals`` has"""
    out = dict(args)
    noise = [a[:n] for a, n in zip(out.pop("_noise"), out_lengths)]
    out["noise"] = noise if isinstance(args["signals"], list) else np.stack(noise)
    return out


def eval_length(n_out):
    return n_out // HOP * HOP - (FRAME - HOP)


def gaps(std):
    """smallest relative difference between neighbouring sorted standard deviations"""
    s = np.sort(np.asarray(std, dtype=np.float64))[::-1]
    return np.inf if len(s) < 2 else float(np.min((s[:-1] - s[1:]) / s[:-1]))


def order_and_gather(y, ref, filler, n_targets, ref_mic, reorder):
    """one room: y (ny, C) float32, ref (K + 1, n_out, M) -> (ref rows (K + 1, m), est rows (K + 1, m), order, std)"""
    std = y.astype(np.float64).std(axis=0)
    order = np.argsort(-std, kind="stable") if reorder else np.arange(y.shape[1])
    if reorder:
        assert gaps(std) > MIN_GAP, f"standard deviations too close for a stable ordering: {std}"
    m = eval_length(ref.shape[1])
    assert m == y.shape[0] - (FRAME - HOP)
    est = np.concatenate([y[:m, order[:n_targets]].T.astype(np.float64), filler[None, :m]])
    return np.ascontiguousarray(ref[:n_targets + 1, :m, ref_mic]), est, order, std


def chain(args, algo, kwargs, monitor=False):
    """-> dict(checkpoints, sdr, sir, sar (B, n_checkpoints, n_targets), perm (B, n_checkpoints, n_targets + 1)) of one algorithm
    entry, by the chain of public calls"""
    import overiva_amd as oa
    from overiva_amd import batch as _batch
    from overiva_amd import pca_batch as _pca_batch

    sim = {k: args[k] for k in ("signals", "room_dim", "sources", "mics", "fs", "max_order", "absorption", "rir_length", "n_targets",
                                "sinr", "snr", "ref_mic", "sources_var", "noise")}
    mix, ref = oa.simulate_batch(**sim)
    mix, ref = list(mix), list(ref)
    B, n_targets, ref_mic = len(mix), args["n_targets"], args["ref_mic"]
    lens = [a.shape[0] for a in mix]
    dense = len(set(lens)) == 1
    x32 = [a.astype(np.float32) for a in mix]
    n_iter, proj_back = kwargs.get("n_iter", 20), kwargs.get("proj_back", True) or algo == "auxiva_pca"
    model = kwargs.get("model", "laplace")
    n_src = {"auxiva": M, "ogive": 1}.get(algo, n_targets)
    reorder = algo not in ("overiva", "ogive", "auxiva_pca")
    marks, evals = [], []
    with oa.BatchSTFT(lens[0] if dense else lens, M, FRAME, HOP, B=B if dense else None) as st:
        Xd = st.analysis_device(np.stack(x32) if dense else x32)

        def evaluate(Yd, reorder):
            y = list(st.synthesis_device(Yd))
            rows = [order_and_gather(y[b], ref[b], args["filler"][b], n_targets, ref_mic, reorder) for b in range(B)]
            sdr, sir, sar, perm = oa.bss_eval_batch([r[0] for r in rows], [r[1] for r in rows], filter_length=LF)
            return sdr, sir, sar, perm

        plan = (_batch.BatchPlan(B, st.frames[0], st.n_freq, M, n_src, model) if dense else
                _batch.RaggedBatchPlan(st.frames, st.n_freq, M, n_src, model))
        with plan:
            plan.set_x_device(Xd.ptr, keepalive=Xd)
            plan.covariance()
            watched = monitor and algo != "auxiva_pca"

            def look(epoch):
                marks.append(epoch)
                evals.append(evaluate(plan.demix_device(proj_back), reorder))

            if not watched:
                marks.append(0)
                evals.append(evaluate(Xd, True))
            if algo == "ogive":
                every_100 = (lambda: look(100 * len(marks))) if watched else None
                _batch._run_ogive(plan, n_iter, None, False, model, every_100=every_100,
                                  **{k: kwargs[k] for k in ("step_size", "tol", "update") if k in kwargs})
            elif algo == "auxiva_pca" and n_src < M:
                _pca_batch.reduce_and_solve(plan, n_iter, None, False, model)
            else:
                plan.set_w(None)
                epoch = 0
                while epoch < n_iter:
                    if watched and epoch % 10 == 0:
                        look(epoch)
                    step = min(n_iter - epoch, 10 - epoch % 10) if watched else n_iter - epoch
                    plan.iterate(step)
                    epoch += step
            look(n_iter)
    out = [np.stack([e[i] for e in evals], axis=1) for i in range(4)]
    return dict(checkpoints=marks, sdr=out[0][:, :, :n_targets], sir=out[1][:, :, :n_targets], sar=out[2][:, :, :n_targets], perm=out[3])


def out_lengths(args):
    """the rooms' output lengths, from the impulse responses of the device"""
    import overiva_amd as oa

    if args["rir_length"] is not None:
        return [np.shape(a)[1] + args["rir_length"] - 1 for a in args["signals"]]
    rirs = oa.rir_batch(args["room_dim"], args["sources"], args["mics"], fs=args["fs"], max_order=args["max_order"],
                        absorption=args["absorption"])
    return [np.shape(a)[1] + h.shape[2] - 1 for a, h in zip(args["signals"], rirs)]


def sweep_args(args):
    """what ``sweep_batch`` takes of a scene that has its noise"""
    return {k: v for k, v in args.items() if not k.startswith("_")}
