"""The reference's command-line driver, src/hmmsort.jl:36-104 (`sort_data`): templates + one
channel of raw data in, decoded state sequence and model out -- the callers either side of the hot
path.

The reference reads HDF5 (`spikeForms`, `cinv`, `p`; data under `rh/data/analogData` or
`highpassdata/data/data`) and writes a MAT file.  h5py is not available in this image, so the
inputs are arrays, `.npz` files or MATLAB v5 `.mat` files with the same variable names; the output
keys and shapes are the reference's (`mlseq`, `ll`, `waveforms`, `lp`, `sigma`, hmmsort.jl:94-98)
and are written with scipy.io.savemat.  Everything between load and save runs through the C ABI.
"""
import numpy as np

from . import api


def get_lp(lA):
    """get_lp(lA::StateMatrix) -> (lp, lidx)   types.jl:42-61: the log-probabilities of the
    transitions silent -> 'exactly one neuron active', in list order, with the neuron index."""
    lp = np.zeros(lA.N)
    lidx = np.zeros(lA.N, dtype=np.int64)
    k = 0
    for src, dst, val in lA.transitions:
        if src == 1 and dst > 1:
            vidx = np.nonzero(lA.states[:, dst - 1] > 1)[0]
            if len(vidx) == 1:
                lp[k] = val
                lidx[k] = vidx[0] + 1
                k += 1
                if k == lA.N:
                    break
    return lp, lidx


def _load(path, names):
    if str(path).endswith(".npz"):
        with np.load(path, allow_pickle=False) as f:
            return {n: f[n] for n in names if n in f}
    from scipy.io import loadmat
    f = loadmat(path)
    return {n: f[n] for n in names if n in f}


def load_templates(path):
    """spikeForms (nstates x nchannels x ntemplates), cinv, p   hmmsort.jl:39-48."""
    d = _load(path, ("spikeForms", "cinv", "p"))
    if "spikeForms" not in d:
        return None          # "No spike forms found. Bailing..."  hmmsort.jl:40-44
    return d["spikeForms"], np.atleast_1d(np.squeeze(d["cinv"])), np.atleast_1d(np.squeeze(d["p"]))


def load_data(path, name="data"):
    d = _load(path, (name,))
    return d[name]


def _chunk_confidence(templates, dataf, ml_seq, chunksize, jitter):
    """spike times and confidences of the decoded path, chunk by chunk of the chunked fit, on the strict path (the
    blocked path under option "engine" = ENGINE_BLOCKED; past its LDS limit with option "blocked_hbm_columns")"""
    n, N = len(ml_seq), templates.state_matrix.N
    times, conf = [[] for _ in range(N)], [[] for _ in range(N)]
    for lo in range(0, n, chunksize):
        hi = min(lo + chunksize, n)
        if hi - lo < 2:
            continue
        part = api.HMMSpikingModel(templates, ml_seq[lo:hi], 0.0, np.asarray(dataf[lo:hi], dtype=np.float64))
        for a, (t, c) in enumerate(api.spike_confidence(part, jitter)):
            times[a].append(t + lo)
            conf[a].append(c)
    cat = lambda parts, dt: [np.concatenate(q) if q else np.zeros(0, dtype=dt) for q in parts]  # noqa: E731
    return cat(times, np.int64), cat(conf, np.float64)


_FRONT_END_KEYS = ("fs", "low", "high", "ntaps", "taps", "reference", "groups", "whiten")
_WHITEN_KEYS = ("threshold", "guard", "thr", "neighbors", "eps_rel")


def _front_end_taps(preprocess):
    """the options of a `preprocess` dictionary and the filter they ask for (None: no filter).  "whiten" comes back
    as None (off), an api.Whitening (applied as it is) or a dictionary of api.whiten's options (estimated from the
    block)."""
    opts = dict(preprocess)
    bad = sorted(set(opts) - set(_FRONT_END_KEYS))
    if bad:
        raise TypeError("preprocess: unknown key(s) %s; known: %s" % (", ".join(bad), ", ".join(_FRONT_END_KEYS)))
    taps = opts.get("taps")
    if taps is None and (opts.get("low") is not None or opts.get("high") is not None):
        if opts.get("fs") is None:
            raise ValueError("preprocess: low / high need the sampling rate fs")
        taps = api.design_fir(opts["fs"], opts.get("low"), opts.get("high"), opts.get("ntaps") or 257)
    wh = opts.get("whiten")
    if wh is None or wh is False:
        opts["whiten"] = None
    elif wh is True:
        opts["whiten"] = {}
    elif not isinstance(wh, api.Whitening):
        opts["whiten"] = dict(wh)
        bad = sorted(set(opts["whiten"]) - set(_WHITEN_KEYS))
        if bad:
            raise TypeError("preprocess: unknown whiten key(s) %s; known: %s" % (", ".join(bad),
                                                                                  ", ".join(_WHITEN_KEYS)))
    return opts, taps


def front_end(data, preprocess, channel=0, info=None):
    """Channel `channel` of the raw block `data` ((T, C) or 1-D) through api.preprocess, as sort_data and
    learn_templates do with their `preprocess` dictionary: either "taps" (the full filter) or "fs" with "low" and / or
    "high" in Hz and "ntaps" (default 257) for api.design_fir; "reference" ("median" or "mean") and "groups" as
    api.preprocess takes them.  An empty dictionary selects and widens the channel, nothing else.

    "whiten": True or a dictionary of api.whiten's options (threshold, guard, thr, neighbors, eps_rel; neighbors may
    also be an int M, the M nearest channels by index) whitens the block after the reference, with the matrix estimated
    from the block itself; an api.Whitening is applied as it is.  The whole block then takes the device path of
    front_end_block (filter, reference, whitening) and row `channel` of it returns.  `info`: a dictionary that receives
    the api.Whitening under "whitening"."""
    opts, taps = _front_end_taps(preprocess)
    if opts["whiten"] is not None:
        d_block = front_end_block(data, preprocess, info)
        if not 0 <= int(channel) < d_block.shape[0]:
            raise ValueError("preprocess: channel = %r of a block of %d channels" % (channel, d_block.shape[0]))
        return d_block[int(channel)].cpu().numpy()
    return api.preprocess(data, taps, opts.get("reference"), opts.get("groups"), keep=[int(channel)])[0]


def front_end_block(data, preprocess, info=None):
    """The whole raw block through the front end, left on the device: the [C][T] float64 tensor of
    device.preprocess, same dictionary and same values as front_end gives channel by channel.  For what looks at a
    unit on every channel (sort_data's `footprints`).  With "whiten" the block is whitened in place on the device
    (device.whiten) and `info["whitening"]` receives the api.Whitening."""
    import torch
    from . import _lib, device
    opts, taps = _front_end_taps(preprocess)
    raw = np.asarray(data)
    if raw.ndim == 1:
        raw = raw[:, None]
    if raw.dtype not in (np.int16, np.int32, np.float32, np.float64):
        raw = raw.astype(np.float64)
    d_raw = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
    d_block = device.preprocess(d_raw, _lib.LAYOUT_SAMPLE_MAJOR, taps, opts.get("reference"), opts.get("groups"))
    wh = opts["whiten"]
    if wh is not None:
        if isinstance(wh, api.Whitening):
            d_block, wh = device.whiten(d_block, whitening=wh, inplace=True)
        else:
            kw = dict(wh)
            if isinstance(kw.get("neighbors"), (int, np.integer)):
                kw["neighbors"] = (np.arange(d_block.shape[0], dtype=np.float64)[:, None], int(kw["neighbors"]))
            d_block, wh = device.whiten(d_block, inplace=True, **kw)
        if info is not None:
            info["whitening"] = wh
    return d_block


def sort_data(spike_forms, cinv, p, data, outputfile=None, dosave=True, max_templates=4,
              chunksize=100_000, confidence=False, jitter=2, refine_steps=0, adapt_halflife=None, quality=False,
              correlograms=None, preprocess=None, channel=0, footprints=None, isolation=None, stability=None):
    """sort_data(inputfile, datafile, outputfile; dosave, max_templates)   hmmsort.jl:36-104.

    Returns the reference's output dictionary; {} when there are more templates than
    `max_templates` (hmmsort.jl:49-52, 57-59).

    `confidence=True` (an extension; default off, output unchanged) adds "spiketimes" (per template, 1-based
    samples as extract_spiketimes) and "confidence" (per spike, api.spike_confidence with `jitter`), computed per
    chunk of the chunked fit from the chunk's own posteriors.  The decode model resolves overlaps, so by default
    this runs on the strict path (alpha and beta materialised, 2 x S x chunksize doubles): slow, and for the 3-
    and 4-template overlap models only feasible with a small `chunksize`.  With option "engine" set to
    ENGINE_BLOCKED the posteriors of a model within the blocked E-step's LDS limit come from the time-parallel
    blocked sweep instead (no S x chunksize array; 2 x 60 at the default chunksize is routine).  Larger models
    -- 3 x 60 and 4 x 60, 10 621 and 21 123 states -- take the same sweep with its state columns in device
    memory when option "blocked_hbm_columns" is 1 as well, at the default chunksize; with that option off (the
    default) they still take the strict path.

    `refine_steps=n` (an extension; default 0, output unchanged) runs n steps of Viterbi training
    (api.viterbi_step) of the overlap model on the channel before the chunked decode: the templates, their entry
    probabilities and sigma are re-estimated from the spikes the model itself sorts, the decode uses the refined
    model, and "waveforms", "lp" and "sigma" in the output are the refined ones.

    `adapt_halflife=h` (an extension; default None, output unchanged) decodes with the drift-tracking loop
    (api.fit_adaptive: the templates and sigma are re-estimated after every chunk from statistics that lose half
    their weight every h samples) and adds "waveforms_track" (chunks x nstates x ntemplates, the templates each chunk
    was decoded with), "sigma_track" and "chunk_first" (1-based first sample of each chunk).  "waveforms" and
    "sigma" stay the model the decode started from.

    `quality=True` (an extension; default off, output unchanged) adds "spiketimes" (when `confidence` has not already),
    "amplitude" and "residual" (per template and spike: api.spike_fit's amp and rss on the whole recording and the
    stitched path) and "unit_quality" (per-template arrays of api.unit_quality's figures).  With `adapt_halflife`
    every spike is measured against the templates its chunk was decoded with.

    `correlograms=True` or a dict of api.correlograms' options (an extension; default None, output unchanged) adds
    "ccg" (templates x templates x 2 half_bins counts of the channel's templates on the stitched path), "ccg_lags"
    (left bin edges in samples) and "isi_violations" (per template).

    `preprocess=dict(...)` (an extension; default None, output unchanged) takes `data` as the raw block of all
    channels: the whole block goes through the front end (front_end: zero-phase FIR filter, common reference) on the
    device and channel `channel` of the result is what gets sorted.  Without it the first column is sorted as it is,
    as in the reference, and `channel` must stay 0.  With "whiten" in the dictionary (front_end) the block is whitened
    after the reference and the output gains the key "whitening": a dictionary of the channel mix ("nbr", "w"), the
    noise scales "sigma" and "n_quiet".  The templates and sigma given must be those of the whitened channel
    (api.Whitening.scale_templates).  Without "whiten" the output is unchanged key for key.

    `footprints=True` or dict(pre=, W=) (an extension; default None, output unchanged; needs `preprocess`) keeps the
    whole preprocessed block on the device instead of one channel of it and adds "footprint" (templates x channels x
    W: the mean waveform of every template on every channel of the block, api.footprints on the stitched path),
    "footprint_n" (spikes used per template) and "peak_channel" (the channel where each template is largest).

    `isolation=True` or dict(pre=, W=, P=, channels=) (an extension; default None, output unchanged) adds
    "unit_isolation": per-template "distance" (isolation distance), "l_ratio", "n_used" and the templates x templates
    "lpair" and "closer" of api.cluster_isolation on the stitched path -- measured on every channel (or `channels`) of
    the preprocessed block, kept on the device, when `preprocess` is given, else on the sorted channel alone.

    `stability=True` or dict(bin=, quantiles=, hist=) (an extension; default None, output unchanged) adds
    "unit_stability": the tables of api.unit_stability on the stitched path's events with api.spike_fit's amplitudes as
    values ("count", "valid", "quant", "sum", "sumsq", "uvalid", "uquant", "umin", "umax", "usum", "usumsq", "hist",
    "under", "over"), "bin" (samples per time bin; default a hundredth of the recording, rounded up), "quantiles" and
    the per-template "presence_ratio", "amplitude_drift" (when 1/2 is among the quantiles) and "amplitude_cutoff"
    (with a histogram; default 512 bins over 0..4 template amplitudes).  With `adapt_halflife` every spike is measured
    against the templates its chunk was decoded with."""
    want_fp = footprints is not None and footprints is not False
    want_iso = isolation is not None and isolation is not False
    if want_fp and preprocess is None:
        raise ValueError("sort_data: footprints needs preprocess (an empty dict takes the block as it is): the "
                         "footprint is measured on every channel of the preprocessed block")
    spike_forms = np.asarray(spike_forms, dtype=np.float64)
    nstates, _nchannels, ntemplates = spike_forms.shape
    pp = np.atleast_1d(np.asarray(p, dtype=np.float64))
    if len(pp) > max_templates:
        return {}
    # StateMatrix(ntemplates, nstates, log.(pp), true): the decode resolves overlaps  :53
    sm = api.StateMatrix.create(ntemplates, nstates, np.log(pp), True)
    sigma = float(np.sqrt(1.0 / np.atleast_1d(cinv)[0]))                      # sqrt(inv(cinv[1])) :55
    templates = api.HMMSpikeTemplateModel(sm, np.asfortranarray(spike_forms[:, 0, :]), sigma)
    lp, _ii = get_lp(sm)                                                       # :61
    data = np.asarray(data)
    d_block, info = None, {}
    if want_fp or (want_iso and preprocess is not None):
        d_block = front_end_block(data, preprocess, info)
        if not 0 <= int(channel) < d_block.shape[0]:
            raise ValueError("sort_data: channel = %r of a block of %d channels" % (channel, d_block.shape[0]))
        data = d_block[int(channel)].cpu().numpy()
    elif preprocess is not None:
        data = front_end(data, preprocess, channel, info)
    elif channel != 0:
        raise ValueError("sort_data: channel = %r needs preprocess (an empty dict selects the channel alone)" % channel)
    if data.ndim == 2:
        data = data[:, 0]                                                      # view(data, :, 1) :80
    # :84-88 converts to Float64 on the host; int16 samples are handed over as they are and widened in HBM
    dataf = np.ascontiguousarray(data) if data.dtype == np.int16 else np.ascontiguousarray(data, dtype=np.float64)
    if refine_steps > 0:
        # raw int16 samples are widened for the refinement only; the decode below still takes them as they are
        em = api._EMSession(np.ascontiguousarray(dataf, dtype=np.float64), hard=True)
        mu_r = np.array(templates.mu, dtype=np.float64, order="F", copy=True)
        try:
            for _ in range(int(refine_steps)):
                sm, mu_r, sigma = em.step(sm, mu_r, sigma)
        finally:
            em.close()
        templates = api.HMMSpikeTemplateModel(sm, mu_r, sigma)
        lp, _ii = get_lp(sm)
    track = None
    if adapt_halflife is not None:
        modelf, track = api.fit_adaptive(templates, dataf, chunksize, float(adapt_halflife))
    else:
        modelf = api.fit(templates, dataf, chunksize)                          # :90
    mlseq = api.unroll_mlseq(modelf.ml_seq, sm)                                # :92
    out = {"mlseq": mlseq, "ll": modelf.ll, "waveforms": templates.mu, "lp": lp, "sigma": sigma}
    if "whitening" in info:
        out["whitening"] = info["whitening"].as_dict()
    if track is not None:
        out["waveforms_track"], out["sigma_track"] = np.ascontiguousarray(track.mu), np.array(track.sigma)
        out["chunk_first"] = np.array(track.first)
    if confidence:
        st, cf = _chunk_confidence(templates, dataf, modelf.ml_seq, chunksize or len(dataf), jitter)
        out["spiketimes"], out["confidence"] = np.empty(len(st), dtype=object), np.empty(len(cf), dtype=object)
        for a in range(len(st)):
            out["spiketimes"][a], out["confidence"][a] = st[a], cf[a]
    if quality:
        fits = api.spike_fit(modelf, track)
        names = (("spiketimes", "times"), ("amplitude", "amp"), ("residual", "rss"))
        for key, field in names[("spiketimes" in out):]:
            out[key] = np.empty(len(fits), dtype=object)                       # a cell per template
            for a, f in enumerate(fits):
                out[key][a] = getattr(f, field)
        uq = [api.quality_from_summary(f.summary, sm.K, sigma) for f in fits]
        out["unit_quality"] = {k: np.array([getattr(q, k) for q in uq])
                               for k in ("n", "n_full", "mean_amp", "sd_amp", "sd_expected", "chi2", "energy")}
        out["unit_quality"]["waveform"] = np.stack([q.waveform for q in uq], axis=1)
        out["unit_quality"]["waveform_sd"] = np.stack([q.waveform_sd for q in uq], axis=1)
    if correlograms is not None and correlograms is not False:
        cg = api.correlograms([modelf], **({} if correlograms is True else dict(correlograms)))
        out["ccg"], out["ccg_lags"], out["isi_violations"] = cg.counts, cg.lags, cg.isi_violations
    if want_fp:
        import torch
        from . import device
        lists = api.extract_spiketimes(modelf)
        offs = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int64)
        d_times = torch.from_numpy(np.concatenate(lists + [np.zeros(0, dtype=np.int64)]).astype(np.int64)).cuda()
        fp = device.footprints(d_block, d_times, offs, **({} if footprints is True else dict(footprints)))
        out["footprint"], out["footprint_n"], out["peak_channel"] = fp.mean, fp.n_used, fp.peak_channel
    if want_iso:
        import torch
        from . import device
        lists = api.extract_spiketimes(modelf)
        offs = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int64)
        d_times = torch.from_numpy(np.concatenate(lists + [np.zeros(0, dtype=np.int64)]).astype(np.int64)).cuda()
        d_iso = d_block if d_block is not None else \
            torch.from_numpy(np.ascontiguousarray(dataf, dtype=np.float64)[None, :]).cuda()
        iso = device.cluster_isolation(d_iso, d_times, offs, **({} if isolation is True else dict(isolation)))
        out["unit_isolation"] = {"distance": iso.distance, "l_ratio": iso.l_ratio, "lpair": iso.lpair,
                                 "closer": iso.closer, "n_used": iso.n_used}
    if stability is not None and stability is not False:
        so = dict(bin=max(1, -(-len(dataf) // 100)), quantiles=(1 / 4, 1 / 2, 3 / 4), hist=(512, 0.0, 4.0))
        so.update({} if stability is True else dict(stability))
        fits = api.spike_fit(modelf, track)
        us = api.unit_stability([f.times for f in fits], [f.amp for f in fits], T=len(dataf), **so)
        d = {k: getattr(us, k) for k in ("count", "valid", "quant", "sum", "sumsq", "uvalid", "uquant", "umin", "umax",
                                         "usum", "usumsq", "hist", "under", "over")}
        d["bin"], d["quantiles"] = us.bin, np.array(us.q_num, dtype=np.float64) / us.q_den
        d["presence_ratio"] = us.presence_ratio()
        if any(2 * q == us.q_den for q in us.q_num):
            d["amplitude_drift"] = us.amplitude_drift()
        if so["hist"] is not None:
            d["amplitude_cutoff"] = us.amplitude_cutoff()
        out["unit_stability"] = d
    if dosave and outputfile is not None:
        from scipy.io import savemat
        savemat(outputfile, out)                                              # MAT.matwrite :100
    return out


def _entry_lp(sm):
    """entry log-probability per template in template order, -Inf where the transition has left the list"""
    lpn = np.full(sm.N, -np.inf)
    lp, lidx = get_lp(sm)
    found = lidx > 0
    lpn[lidx[found] - 1] = lp[found]
    return lpn


def merge_and_prune(sm, mu, sigma):
    """The reference's stage between the two rounds of steps (condense_templates, remove_sparse, remove_small,
    baumwelch.jl:340-349) for either kind of model.  The reference runs it on the model it trains, which has no
    overlaps; an overlap model goes through it as the no-overlap model of the same templates and entry
    probabilities and is rebuilt from what is left."""
    from .postprocess import reference_postprocess
    if not sm.resolve_overlaps:
        return reference_postprocess(sm, mu, sigma)
    ring, mu = reference_postprocess(api.StateMatrix.create(sm.N, sm.K, _entry_lp(sm), False), mu, sigma)
    if ring.N == 0:
        return ring, mu
    return api.StateMatrix.create(ring.N, sm.K, _entry_lp(ring), True), mu


def learn_templates(data, N=3, K=60, nsteps=4, method="viterbi", resolve_overlaps=True, postprocess=merge_and_prune,
                    seed_options=None, preprocess=None, channel=0):
    """The learning stage in front of sort_data (an extension: the reference takes its templates from a file an
    earlier stage wrote): seed N templates of K states from the channel's threshold crossings (api.seed_templates)
    and train them with api.train_model(..., init="detect"); `postprocess` is train_model's (default: the reference's
    merge-and-prune stage, see merge_and_prune).  Returns the dictionary sort_data takes: "spikeForms" (K, 1, n),
    "cinv" [1 / sigma^2] and "p" (entry probability per template), n <= N being the templates that are left with a
    finite entry transition.  `preprocess`, `channel`: as in sort_data; with "whiten" the templates are those of the
    whitened channel and the dictionary gains the key "whitening" as sort_data's output does."""
    data = np.asarray(data)
    info = {}
    if preprocess is not None:
        data = front_end(data, preprocess, channel, info)
    elif channel != 0:
        raise ValueError("learn_templates: channel = %r needs preprocess (an empty dict selects the channel alone)"
                         % channel)
    if data.ndim == 2:
        data = data[:, 0]
    X = np.ascontiguousarray(data, dtype=np.float64)
    sm, mu, sigma = api.train_model(X, int(N), int(K), bool(resolve_overlaps), int(nsteps), method=method,
                                    init="detect", postprocess=postprocess, seed_options=seed_options)
    p = np.exp(_entry_lp(sm)) if sm.N > 0 else np.zeros(0)
    keep = np.nonzero(p > 0)[0]
    mu = np.asarray(mu, dtype=np.float64).reshape(int(K), -1)
    out = {"spikeForms": np.ascontiguousarray(mu[:, keep][:, None, :]), "cinv": np.array([1.0 / (sigma * sigma)]),
           "p": p[keep]}
    if "whitening" in info:
        out["whitening"] = info["whitening"].as_dict()
    return out


def main(argv=None):
    """The command line.  With --whiten and --learn the learning stage and the sort each run the front end on the
    block: every stage is deterministic, so the same whitening matrix is estimated twice, to the bit."""
    import argparse
    ap = argparse.ArgumentParser(description="HMM spike sorting of one channel (hmmsort.jl CLI)")
    ap.add_argument("--sourcefile", help=".npz/.mat with spikeForms, cinv, p (not needed with --learn)")
    ap.add_argument("--learn", type=int, default=0, metavar="N",
                    help="learn up to N templates from the data itself instead of reading --sourcefile")
    ap.add_argument("--nstates", type=int, default=60, help="template length for --learn")
    ap.add_argument("--datafile", required=True, help=".npz/.mat with the channel's samples")
    ap.add_argument("--dataname", default="data")
    ap.add_argument("--outfile", default="hmmsort.mat")
    ap.add_argument("--max_templates", type=int, default=4)
    ap.add_argument("--fs", type=float, help="sampling rate in Hz (with --highpass / --lowpass)")
    ap.add_argument("--highpass", type=float, metavar="HZ", help="zero-phase FIR filter: pass above HZ")
    ap.add_argument("--lowpass", type=float, metavar="HZ", help="zero-phase FIR filter: pass below HZ")
    ap.add_argument("--ntaps", type=int, default=257, help="filter length (odd)")
    ap.add_argument("--reference", choices=("median", "mean"),
                    help="subtract the common reference of all channels of the block, per sample")
    ap.add_argument("--channel", type=int, default=0, help="column of the raw block to sort (0-based)")
    ap.add_argument("--whiten", action="store_true",
                    help="whiten the block across channels after the reference (noise covariance of its quiet samples)")
    ap.add_argument("--whiten-threshold", type=float, default=4.0, metavar="X",
                    help="a sample beyond X noise scales on any channel is not quiet")
    ap.add_argument("--whiten-guard", type=int, default=30, metavar="N", help="nor are the N samples either side of it")
    ap.add_argument("--whiten-neighbors", type=int, metavar="M",
                    help="local whitening: each channel against its M nearest by channel index (default: all)")
    ap.add_argument("--isolation", action="store_true",
                    help="add unit_isolation (isolation distance, L-ratio) of the sorted templates to the output")
    ap.add_argument("--stability", action="store_true",
                    help="add unit_stability (counts and amplitude quantiles per time bin, presence ratio, amplitude "
                         "drift and cutoff) of the sorted templates to the output")
    ap.add_argument("--stability-bin", type=int, metavar="N",
                    help="samples per time bin of --stability (default: a hundredth of the recording)")
    a = ap.parse_args(argv)
    pre = None
    if a.highpass is not None or a.lowpass is not None or a.reference is not None or a.channel != 0 or a.whiten:
        if (a.highpass is not None or a.lowpass is not None) and a.fs is None:
            ap.error("--highpass / --lowpass need --fs")
        pre = {"fs": a.fs, "low": a.highpass, "high": a.lowpass, "ntaps": a.ntaps, "reference": a.reference}
        if a.whiten:
            pre["whiten"] = {"threshold": a.whiten_threshold, "guard": a.whiten_guard,
                             "neighbors": a.whiten_neighbors}
    data = None
    if a.learn > 0:
        data = load_data(a.datafile, a.dataname)
        d = learn_templates(data, a.learn, a.nstates, preprocess=pre, channel=a.channel)
        t = (d["spikeForms"], d["cinv"], d["p"]) if len(d["p"]) else None
    elif a.sourcefile is None:
        ap.error("--sourcefile is required without --learn")
    else:
        t = load_templates(a.sourcefile)
    if t is None:
        print("No spike forms found. Bailing...")
        return 0
    if data is None:
        data = load_data(a.datafile, a.dataname)
    out = sort_data(*t, data, a.outfile, max_templates=a.max_templates, preprocess=pre, channel=a.channel,
                    isolation=True if a.isolation else None,
                    stability=(dict(bin=a.stability_bin) if a.stability_bin else True) if a.stability else None)
    print("Done! Results saved to %s" % a.outfile if out else "Too many templates. Bailing out...")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
