"""Rate of the reference CLI's decode: fit(HMMSpikingModel, templates, X, 100_000) (fit.jl:11-42,
hmmsort.jl:90) on an overlap-resolving model, host array in, host array out: the host loop api.fit, the native
loop hmmsort_fit_chunked, and hmmsort_fit_channels with 4 and 8 equal channels at fit_streams 1 and 4.
Median of 5 after one warm-up.   python scripts/bench_fit.py [T [N]]"""
import sys, time
sys.path.insert(0, ".")
import numpy as np
import hmmsort_amd as H

K = 60
N = int(sys.argv[2]) if len(sys.argv) > 2 else 2
shapes = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
temps = np.asfortranarray(np.stack([H.create_spike_template(K, *shapes[i]) for i in range(N)], 1))
pp = [0.003, 0.001, 0.002, 0.0015][:N]
sm = H.StateMatrix.create(N, K, np.log(pp), True)
T = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
CHUNK = 100_000
y = H.create_signal(T, 0.3, pp, temps, seed=3)
tm = H.HMMSpikeTemplateModel(sm, temps, 0.3)


def median_of_5(f):
    f()                                  # warm-up: plans, buffers, code objects
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), out


dt, m = median_of_5(lambda: H.fit(tm, y, CHUNK))
print("api.fit (host loop), N=%d K=60 overlaps (%d states), %d samples in 100k chunks: %.3f s = %.1f Msamples/s"
      % (N, sm.nstates, T, dt, T / dt / 1e6))
dt, m1 = median_of_5(lambda: H.fit_channels(tm, [y], CHUNK)[0])
print("hmmsort_fit_chunked (native loop): %.3f s = %.1f Msamples/s, escalations %d; same path as api.fit: %s; "
      "ll (folded serially, as the reference rounds it) - api.fit's ll (summed in parts): %.3g relative"
      % (dt, T / dt / 1e6, H.get_option("last_escalations"), np.array_equal(m.ml_seq, m1.ml_seq),
         (m1.ll - m.ll) / abs(m.ll)))
for nch in (4, 8):
    for streams in (1, 4):
        H.set_option("fit_streams", streams)
        dt, ms = median_of_5(lambda: H.fit_channels(tm, [y] * nch, CHUNK))
        same = all(np.array_equal(q.ml_seq, m1.ml_seq) and q.ll == m1.ll for q in ms)
        print("hmmsort_fit_channels, %d equal channels, fit_streams %d: %.3f s = %.1f Msamples/s aggregate; every "
              "channel equal to the single one: %s" % (nch, streams, dt, nch * T / dt / 1e6, same))
H.set_option("fit_streams", 4)
t = time.time(); m2 = H.fit(tm, y); dt = time.time() - t
print("whole-signal decode through hmmsort_viterbi: %.3f s = %.1f Msamples/s; same path as chunked: %s"
      % (dt, T / dt / 1e6, np.array_equal(m.ml_seq, m2.ml_seq)))
for rep in range(3):
    t = time.time(); x, ll = H.viterbi(y, sm, temps, 0.3); dt = time.time() - t
    print("hmmsort_viterbi call %d: %.3f s = %.1f Msamples/s (escalations %d)" % (rep, dt, T / dt / 1e6, H.get_option("last_escalations")))
H.shutdown()
