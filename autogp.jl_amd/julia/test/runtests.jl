# Parity tests of the ccall shim against AutoGP.jl's OWN Julia path, for a maintainer with Julia + Gen + AutoGP.jl and
# an MI355X:   ] dev <AutoGP.jl>  ;  ] dev autogp.jl_amd/julia  ;  ] build AutoGPHIP  ;  ] test AutoGPHIP
#
# STATUS: never executed (no Julia in the build image nor on the GPU box).  They restate, against the reference's own
# functions, what tests/test_gpu_*.py check through ctypes against the oracle: the day this file runs green the
# "parity unpinned" caveat of DESIGN.md §6 goes away.  Tolerances are north_star's: 1e-8 relative on logpdf.
using Test, Random, LinearAlgebra
import AutoGP, Gen, Distributions
import AutoGPHIP
const GP = AutoGP.GP
const H = AutoGPHIP

relerr(a, b) = abs(a - b) / max(1.0, abs(b))
maxrel(a, b) = maximum(abs.(a .- b)) / max(1.0, maximum(abs.(b)))

"the reference's own score of `xs` (src/Model.jl:135-136)"
ref_logpdf(node, noise, ts, xs) =
    Gen.logpdf(Gen.mvnormal, xs, zeros(length(ts)), GP.compute_cov_matrix_vectorized(node, noise, ts))

function series(n; seed=1)
    rng = MersenneTwister(seed)
    ts = sort(rand(rng, n))
    xs = 0.6 .* sin.(9.0 .* ts) .+ 0.4 .* ts .+ 0.15 .* randn(rng, n)
    return ts, xs
end

kernels() = GP.Node[
    GP.Linear(0.1, 0.3, 0.7),
    GP.SquaredExponential(0.21, 0.9),
    GP.GammaExponential(0.33, 1.4, 0.8),
    GP.Periodic(0.96, 0.21, 1.1),
    GP.Constant(0.4) + GP.WhiteNoise(0.2),
    GP.Linear(0.1, 0.3, 0.7) + GP.Periodic(0.96, 0.21, 1.1) * GP.SquaredExponential(0.47, 0.8),
    GP.ChangePoint(GP.SquaredExponential(0.2, 1.0), GP.Periodic(0.5, 0.3, 0.6), 0.45, 0.001),
    GP.ChangePoint(GP.Linear(0.0, 0.2, 0.5) * GP.GammaExponential(0.4, 0.9, 1.2),
                   GP.ChangePoint(GP.Constant(0.3), GP.SquaredExponential(0.1, 0.5), 0.8, 0.001) + GP.Periodic(0.7, 0.15, 0.9),
                   0.3, 0.001),
]

@testset "AutoGPHIP" begin
    eng = H.Engine(0)
    ts, xs = series(700)
    H.set_data!(eng, ts, xs)
    noise = 0.07 + 1e-5            # the value AFTER + JITTER, as the model body passes it

    @testset "program round trip" begin
        for k in kernels()
            ops, th = H.encode(k)
            k2 = H.node_from_flat(ops, th)
            @test GP.eval_cov(k2, ts[1:40]) == GP.eval_cov(k, ts[1:40])
            @test length(ops) == length(GP.unroll(k))
        end
    end

    @testset "logpdf vs mvnormal (n = $n)" for n in (1, 2, 17, 127, 128, 129, 300, 700)
        for k in kernels()
            @test relerr(H.logpdf(eng, k, noise, n), ref_logpdf(k, noise, ts[1:n], xs[1:n])) <= 1e-8
        end
    end

    @testset "batch entry, resident factors along a schedule" begin
        ks = kernels(); nz = fill(noise, length(ks))
        for n in (130, 300, 301, 700)
            a, ia = H.logpdf_batch(eng, ks, nz, n)
            b, ib = H.logpdf_batch(eng, ks, nz, n; extend=true)
            @test all(ia .== 0) && all(ib .== 0)
            for (i, k) in enumerate(ks)
                r = ref_logpdf(k, noise, ts[1:n], xs[1:n])
                @test relerr(a[i], r) <= 1e-8
                @test relerr(b[i], r) <= 1e-8
            end
        end
    end

    @testset "many short series in one call (stateless)" begin
        ks = kernels()
        sers = [(ts[1:n], xs[1:n]) for n in (0, 1, 17, 144, H.SERIES_MAX_N)]
        nodes = GP.Node[]; sidx = Int[]
        for s in eachindex(sers), k in ks
            push!(nodes, k); push!(sidx, s)
        end
        lp, info = H.logpdf_series_batch(eng, sers, nodes, fill(noise, length(nodes)), sidx)
        @test all(info .== 0)
        for (p, (k, s)) in enumerate(zip(nodes, sidx))
            t, x = sers[s]
            @test relerr(lp[p], isempty(t) ? 0.0 : ref_logpdf(k, noise, t, x)) <= 1e-8
        end
        @test eng.n_max == 700      # the resident series is untouched
    end

    @testset "series of up to LONG_SERIES_MAX_N points in one call (stateless)" begin
        ks = kernels()
        sers = [(ts[1:n], xs[1:n]) for n in (0, 17, 143, H.SERIES_MAX_N, H.SERIES_MAX_N + 1, 442, H.LONG_SERIES_MAX_N)]
        nodes = GP.Node[]; sidx = Int[]
        for s in eachindex(sers), k in ks
            push!(nodes, k); push!(sidx, s)
        end
        nz = fill(noise, length(nodes))
        lp, info = H.logpdf_long_series_batch(eng, sers, nodes, nz, sidx)
        la, ia = H.logpdf_long_series_batch(eng, sers, nodes, nz, sidx; all_long=true)
        @test all(info .== 0) && all(ia .== 0)
        for (p, (k, s)) in enumerate(zip(nodes, sidx))
            t, x = sers[s]
            r = isempty(t) ? 0.0 : ref_logpdf(k, noise, t, x)
            @test relerr(lp[p], r) <= 1e-8
            @test relerr(la[p], r) <= 1e-8
        end
        # up to the short cap the default routing is logpdf_series_batch's kernel: the same bits
        short = [p for p in eachindex(nodes) if length(sers[sidx[p]][1]) <= H.SERIES_MAX_N]
        ls, _ = H.logpdf_series_batch(eng, sers[1:4], nodes[short], nz[short], sidx[short])
        @test lp[short] == ls
        @test_throws ArgumentError H.logpdf_long_series_batch(eng, [(zeros(513), zeros(513))], ks[1:1], [noise], [1])
        @test eng.n_max == 700      # the resident series is untouched
    end

    @testset "many short series: held-out scores in one call (stateless)" begin
        ks = kernels()
        splits = ((0, 5), (17, 5), (126, 18), (144, 32))      # (training points, held-out points)
        sers = [(ts[1:n], xs[1:n]) for (n, _) in splits]
        qs = [ts[n + 1:n + m] for (n, m) in splits]
        a, b = 0.7, -0.2                                       # scaled = a raw + b
        held = [(xs[n + 1:n + m] .- b) ./ a for (n, m) in splits]
        nodes = GP.Node[]; sidx = Int[]
        for s in eachindex(sers), k in ks
            push!(nodes, k); push!(sidx, s)
        end
        P = length(nodes)
        w = Float64[1 / length(ks) for _ in 1:P]
        lp, terms, mix, info = H.predict_proba_series_batch(eng, sers, qs, held, nodes, fill(noise, P), sidx; weights=w,
                                                            y_transforms=fill((a, b), length(sers)))
        @test all(info .== 0)
        for (p, (k, s)) in enumerate(zip(nodes, sidx))
            n, m = splits[s]
            # the chain rule with noise_pred = noise: log p(joint) - log p(training part), plus the Jacobian of the transform
            r = ref_logpdf(k, noise, ts[1:n + m], xs[1:n + m]) - (n == 0 ? 0.0 : ref_logpdf(k, noise, ts[1:n], xs[1:n])) + m * log(a)
            @test relerr(lp[p], r) <= 1e-7
            @test length(terms[p]) == m && relerr(sum(terms[p]), lp[p]) <= 1e-12
        end
        for s in eachindex(sers)
            sel = findall(==(s), sidx)
            M = maximum(lp[sel])
            @test relerr(mix[s], M + log(sum(w[sel] .* exp.(lp[sel] .- M)))) <= 1e-12
        end
        @test eng.n_max == 700      # the resident series is untouched
    end

    @testset "series of up to 512 joint points: held-out scores in one call (stateless)" begin
        ks = kernels()
        splits = ((0, 5), (126, 18), (144, 36), (406, 36))     # (training points, held-out points): joint lengths 5, 144, 180, 442
        sers = [(ts[1:n], xs[1:n]) for (n, _) in splits]
        qs = [ts[n + 1:n + m] for (n, m) in splits]
        a, b = 0.7, -0.2                                       # scaled = a raw + b
        held = [(xs[n + 1:n + m] .- b) ./ a for (n, m) in splits]
        nodes = GP.Node[]; sidx = Int[]
        for s in eachindex(sers), k in ks
            push!(nodes, k); push!(sidx, s)
        end
        P = length(nodes)
        w = Float64[1 / length(ks) for _ in 1:P]
        yts = fill((a, b), length(sers))
        lp, terms, mix, info = H.predict_proba_long_series_batch(eng, sers, qs, held, nodes, fill(noise, P), sidx; weights=w, y_transforms=yts)
        la, _, _, ia = H.predict_proba_long_series_batch(eng, sers, qs, held, nodes, fill(noise, P), sidx; weights=w, y_transforms=yts,
                                                         all_long=true)
        @test all(info .== 0) && all(ia .== 0)
        for (p, (k, s)) in enumerate(zip(nodes, sidx))
            n, m = splits[s]
            r = ref_logpdf(k, noise, ts[1:n + m], xs[1:n + m]) - (n == 0 ? 0.0 : ref_logpdf(k, noise, ts[1:n], xs[1:n])) + m * log(a)
            @test relerr(lp[p], r) <= 1e-7
            @test relerr(la[p], r) <= 1e-7
            @test length(terms[p]) == m && relerr(sum(terms[p]), lp[p]) <= 1e-12
        end
        # up to the short cap on the joint length the default routing is predict_proba_series_batch's kernel: the same bits
        short = [p for p in eachindex(nodes) if sum(splits[sidx[p]]) <= H.SERIES_MAX_N]
        ls, _, ms, _ = H.predict_proba_series_batch(eng, sers[1:2], qs[1:2], held[1:2], nodes[short], fill(noise, length(short)),
                                                    sidx[short]; weights=w[short], y_transforms=yts[1:2])
        @test lp[short] == ls && mix[1:2] == ms
        @test_throws ArgumentError H.predict_proba_long_series_batch(eng, [(ts[1:500], xs[1:500])], [ts[501:513]], [xs[501:513]], ks[1:1],
                                                                     [noise], [1])
        @test eng.n_max == 700      # the resident series is untouched
    end

    @testset "many short series: sample paths and joint forecasts in one call (stateless)" begin
        ks = kernels()
        splits = ((0, 5), (17, 5), (126, 18), (140, 36))       # (training points, query points)
        sers = [(ts[1:n], xs[1:n]) for (n, _) in splits]
        qs = [ts[n + 1:n + m] for (n, m) in splits]
        a, b = -0.7, 0.2                                       # scaled = a raw + b
        nodes = GP.Node[]; sidx = Int[]
        for s in eachindex(sers), k in ks
            push!(nodes, k); push!(sidx, s)
        end
        P = length(nodes); R = 50
        w = Float64[1 / length(ks) for _ in 1:P]
        seeds = UInt64[11, 12, 13, 14]
        yts = fill((a, b), length(sers))
        x, comp, means, covs, info = H.predict_rand_series_batch(eng, sers, qs, nodes, fill(noise, P), sidx, w, R, seeds;
                                                                 y_transforms=yts, want_moments=true)
        @test all(info .== 0)
        mu2, cv2, info2 = H.predict_mvn_series_batch(eng, sers, qs, nodes, fill(noise, P), sidx, w; y_transforms=yts)
        @test mu2 == means && cv2 == covs && info2 == info     # the moments do not depend on the samples drawn beside them
        for (p, (k, s)) in enumerate(zip(nodes, sidx))
            n, m = splits[s]
            # the posterior predictive in raw space from the dense formulas
            K = GP.compute_cov_matrix_vectorized(k, noise, vcat(ts[1:n], qs[s]))
            K11, K21, K22 = K[1:n, 1:n], K[n + 1:end, 1:n], K[n + 1:end, n + 1:end]
            mu = n == 0 ? zeros(m) : K21 * (K11 \ xs[1:n])
            Sg = n == 0 ? K22 : K22 - K21 * (K11 \ K21')
            @test maximum(abs.(means[p] .- (mu .- b) ./ a)) <= 1e-8 * max(1.0, maximum(abs.(mu ./ a)))
            @test norm(covs[p] - Sg ./ a^2) <= 1e-8 * norm(Sg ./ a^2)
            @test covs[p] == covs[p]'
        end
        for s in eachindex(sers)
            sel = findall(==(s), sidx)
            @test size(x[s]) == (splits[s][2], R) && all(c -> c in sel, comp[s]) && all(isfinite, x[s])
        end
        # series 3 alone under its own seed: the same bits
        sel = findall(==(3), sidx)
        x3, comp3, _, _, _ = H.predict_rand_series_batch(eng, [sers[3]], [qs[3]], nodes[sel], fill(noise, length(sel)),
                                                         fill(1, length(sel)), w[sel], R, seeds[3:3]; y_transforms=yts[3:3])
        @test x3[1] == x[3] && comp3[1] .+ (sel[1] - 1) == comp[3]
        # 144 training points + 36 queries are 180 joint points: refused
        @test_throws ErrorException H.predict_rand_series_batch(eng, [(ts[1:144], xs[1:144])], [ts[145:180]], nodes[1:1], [noise], [1],
                                                                [1.0], 1, UInt64[1])
        @test eng.n_max == 700      # the resident series is untouched
    end

    @testset "many short series: decompositions in one call (stateless)" begin
        ks = kernels()[[6, 7, 8]]
        shapes = ((0, 5), (17, 6), (126, 12), (144, 36))       # (training points, query points)
        sers = [(ts[1:n], xs[1:n]) for (n, _) in shapes]
        qs = [ts[n + 1:n + m] for (n, m) in shapes]
        yts = [(1.0 + 0.5 * s, 0.1 * s) for s in eachindex(sers)]
        quantiles = [0.025, 0.5, 0.975]
        splits = []; sidx = Int[]
        for s in eachindex(sers), k in ks
            push!(splits, collect(GP.split_kernel_sop(k, GP.Periodic))); push!(sidx, s)
        end
        P = length(splits)
        means, vars, x, lp, info = H.predict_sum_series_batch(eng, sers, qs, splits, fill(noise, P), sidx; quantiles=quantiles,
                                                              y_transforms=yts)
        @test all(info .== 0)
        for (p, s) in enumerate(sidx)
            n, m = shapes[s]
            a, b = yts[s]
            @test length(means[p]) == 3m && size(x[p]) == (3, 3m)
            @test x[p][2, :] == means[p]                       # the median of a Normal is its mean: fma(sd, 0, mean)
            @test all(x[p][1, :] .<= means[p]) && all(means[p] .<= x[p][3, :])
            n == 0 && continue
            # the reference's route on the series' own data
            mu, S, _ = GP.infer_gp_sum(splits[p], noise, ts[1:n], xs[1:n], qs[s])
            mr = (mu .- b) ./ a
            mr[1:m] .+= b / a
            @test maximum(abs.(means[p] .- mr)) <= 1e-8 * max(1.0, maximum(abs.(mr)))
            @test maximum(abs.(vars[p] .- diag(S) ./ a^2)) <= 1e-8 * max(1.0, maximum(abs.(diag(S) ./ a^2)))
        end
        # series 3 alone: the same bits
        sel = findall(==(3), sidx)
        m3, v3, x3, _, _ = H.predict_sum_series_batch(eng, [sers[3]], [qs[3]], splits[sel], fill(noise, length(sel)),
                                                      fill(1, length(sel)); quantiles=quantiles, y_transforms=yts[3:3])
        @test m3 == means[sel] && v3 == vars[sel] && x3 == x[sel]
        @test eng.n_max == 700      # the resident series is untouched
    end

    @testset "not positive definite" begin
        bad = GP.Linear(0.0, 0.0, -0.01)
        @test_throws LinearAlgebra.PosDefException H.logpdf(eng, bad, 0.1, 700)
        @test_throws LinearAlgebra.PosDefException ref_logpdf(bad, 0.1, ts, xs)
    end

    @testset "predictive vs Distributions.MvNormal(node, ...)" begin
        tp = vcat(ts[1:5:end], collect(range(1.0, 1.3; length=40)))
        for k in kernels(), np in (nothing, 0.0)
            d = H.predict_mvn(eng, k, noise, tp; noise_pred=np)
            r = Distributions.MvNormal(k, noise, ts, xs, tp; noise_pred=np)
            @test maxrel(Distributions.mean(d), Distributions.mean(r)) <= 1e-8
            @test maxrel(Matrix(Distributions.cov(d)), Matrix(Distributions.cov(r))) <= 1e-8
            mu, v = H.predict_marginal(eng, k, noise, tp; noise_pred=np)
            @test maxrel(mu, Distributions.mean(r)) <= 1e-8
            @test maxrel(v, diag(Matrix(Distributions.cov(r)))) <= 1e-8
            for p in (0.1, 0.5, 0.9)
                @test maxrel(Distributions.quantile(d, p), Distributions.quantile(r, p)) <= 1e-8
            end
        end
        # a mean function (test/test_api.jl of the reference uses one)
        f = t -> 0.3 + 0.1 * t
        k = kernels()[6]
        d = H.predict_mvn(eng, k, noise, tp; mean_train=f.(ts), mean_pred=f.(tp))
        r = Distributions.MvNormal(k, noise, ts, xs, tp; mean=f)
        @test maxrel(Distributions.mean(d), Distributions.mean(r)) <= 1e-8
        # the predictive call after an extension sweep on the same prefix starts from the resident factor
        H.logpdf_batch(eng, GP.Node[k], [noise], 700; extend=true)
        before = H.predict_reuse_stats(eng).reused
        d2 = H.predict_mvn(eng, k, noise, tp)
        @test H.predict_reuse_stats(eng).reused == before + 1
        @test maxrel(Distributions.mean(d2), Distributions.mean(Distributions.MvNormal(k, noise, ts, xs, tp))) <= 1e-8
    end

    @testset "moments of predict_mvn's MixtureModel, and of its MvLogNormal re-wrap" begin
        # (predict_mvn builds exactly this: MixtureModel of the particles' MvNormals with the particle weights, src/api.jl:508-521)
        tp = vcat(ts[1:25:end], collect(range(1.0, 1.2; length=20)))
        ks = GP.Node[k for k in kernels()[1:4]]
        nz = fill(noise, length(ks))
        w = collect(1.0:length(ks)); w ./= sum(w)
        comps = [Distributions.MvNormal(k, noise, ts, xs, tp) for k in ks]
        r = Distributions.MixtureModel(comps, w)
        mu, v, C = H.predict_mvn_moments(eng, ks, nz, w, tp)
        @test maxrel(mu, Distributions.mean(r)) <= 1e-8
        @test maxrel(v, Distributions.var(r)) <= 1e-8
        @test maxrel(C, Matrix(Distributions.cov(r))) <= 1e-8
        @test C == C' && v == diag(C)
        mu0, v0, C0 = H.predict_mvn_moments(eng, ks, nz, w, tp; want_cov=false)
        @test isnothing(C0) && maxrel(mu0, Distributions.mean(r)) <= 1e-8 && maxrel(v0, Distributions.var(r)) <= 1e-8
        rl = Distributions.MixtureModel([Distributions.MvLogNormal(c) for c in comps], w)
        mul, vl, Cl = H.predict_mvn_moments(eng, ks, nz, w, tp; lognormal=true)
        @test maxrel(mul, Distributions.mean(rl)) <= 1e-8
        @test maxrel(vl, Distributions.var(rl)) <= 1e-8
        @test maxrel(Cl, Matrix(Distributions.cov(rl))) <= 1e-8
    end

    @testset "infer_gp_sum" begin
        nodes = GP.Node[GP.Linear(0.1, 0.3, 0.7), GP.Periodic(0.96, 0.21, 1.1), GP.SquaredExponential(0.3, 0.5)]
        tp = collect(range(0.0, 1.2; length=25))
        a = H.infer_gp_sum(eng, nodes, noise, tp)
        b = GP.infer_gp_sum(nodes, noise, ts, xs, tp)
        @test a.indexes.F == b.indexes.F && a.indexes.X == b.indexes.X
        @test maxrel(Distributions.mean(a.mvn), Distributions.mean(b.mvn)) <= 1e-8
        @test maxrel(Matrix(Distributions.cov(a.mvn)), Matrix(Distributions.cov(b.mvn))) <= 1e-8
    end

    @testset "gradient vs central differences of the reference's score" begin
        n = 300
        for k in kernels()
            ops, th = H.encode(k)
            lp, g, gn = H.logpdf_grad(eng, k, noise, n)
            @test relerr(lp, ref_logpdf(k, noise, ts[1:n], xs[1:n])) <= 1e-8
            f(thv, nz) = ref_logpdf(H.node_from_flat(ops, thv), nz, ts[1:n], xs[1:n])
            for j in eachindex(th)
                h = 1e-6 * max(1.0, abs(th[j]))
                tp_ = copy(th); tm_ = copy(th); tp_[j] += h; tm_[j] -= h
                fd = (f(tp_, noise) - f(tm_, noise)) / (2h)
                @test abs(g[j] - fd) <= 1e-5 * max(1.0, abs(fd))
            end
            h = 1e-7
            @test abs(gn - (f(th, noise + h) - f(th, noise - h)) / (2h)) <= 1e-4 * max(1.0, abs(gn))
        end
    end

    @testset "many short series: value and gradient in one call (stateless)" begin
        ks = kernels()
        sers = [(ts[1:n], xs[1:n]) for n in (0, 17, 144)]
        nodes = GP.Node[]; sidx = Int[]
        for s in eachindex(sers), k in ks
            push!(nodes, k); push!(sidx, s)
        end
        nz = fill(noise, length(nodes))
        lp, grads, gn, info = H.logpdf_grad_series_batch(eng, sers, nodes, nz, sidx)
        lp_v, _ = H.logpdf_series_batch(eng, sers, nodes, nz, sidx)
        @test all(info .== 0)
        @test lp == lp_v                                        # the value is the value entry's, bit for bit
        for (p, (k, s)) in enumerate(zip(nodes, sidx))
            t, x = sers[s]
            ops, th = H.encode(k)
            @test length(grads[p]) == length(th)
            if isempty(t)
                @test lp[p] == 0.0 && all(grads[p] .== 0.0) && gn[p] == 0.0
                continue
            end
            f(thv, z) = ref_logpdf(H.node_from_flat(ops, thv), z, t, x)
            for j in eachindex(th)
                h = 1e-6 * max(1.0, abs(th[j]))
                tp_ = copy(th); tm_ = copy(th); tp_[j] += h; tm_[j] -= h
                fd = (f(tp_, noise) - f(tm_, noise)) / (2h)
                @test abs(grads[p][j] - fd) <= 1e-5 * max(1.0, abs(fd))
            end
            h = 1e-7
            @test abs(gn[p] - (f(th, noise + h) - f(th, noise - h)) / (2h)) <= 1e-4 * max(1.0, abs(gn[p]))
        end
        @test eng.n_max == 700      # the resident series is untouched
    end

    @testset "many short series: HMC rejuvenation in one call (stateless)" begin
        ks = kernels()
        sers = [(ts[1:n], xs[1:n]) for n in (17, 144)]
        nodes = GP.Node[]; sidx = Int[]
        for s in eachindex(sers), k in ks
            push!(nodes, k); push!(sidx, s)
        end
        nz = fill(noise, length(nodes))
        seeds = collect(1:length(nodes))
        cfg = Dict(:L_param => 3, :L_noise => 3)
        moved, nz1, lp, counts, info = H.mcmc_parameters_series_batch(eng, sers, nodes, nz, sidx, 3, seeds; hmc_config = cfg)
        @test all(info .== 0) && all(counts[2, :] .== 3)
        lp_v, _ = H.logpdf_series_batch(eng, sers, moved, nz1, sidx)
        @test lp == lp_v                                        # the value entry's bits at the moved state
        for (p, (k, s)) in enumerate(zip(moved, sidx))          # ... and the reference's own score there
            t, x = sers[s]
            @test abs(lp[p] - ref_logpdf(k, nz1[p], t, x)) <= 1e-8 * max(1.0, abs(lp[p]))
            @test H.structure(k) == H.structure(nodes[p])
        end
        again = H.mcmc_parameters_series_batch(eng, sers, nodes, nz, sidx, 3, seeds; hmc_config = cfg)
        @test again[3] == lp && again[2] == nz1                 # a particle's chain depends on its seed and inputs only
        same, nz0, lp0, c0, _ = H.mcmc_parameters_series_batch(eng, sers, nodes, nz, sidx, 0, seeds)
        @test all(c0 .== 0) && all(abs.(nz0 .- nz) .<= 1e-12)
        @test eng.n_max == 700      # the resident series is untouched
    end

    @testset "Gen: value and gradient through gp_marginal_flat; HMC reuses the value call's factor" begin
        k0 = GP.Linear(0.1, 0.3, 0.7) + GP.Periodic(0.96, 0.21, 1.1) * GP.SquaredExponential(0.47, 0.8)
        ops = H.structure(k0)
        np_ = length(H.flat_params(k0))
        Gen.@gen function toy(ts::Vector{Float64})
            z = Vector{Real}(undef, np_)
            for j in 1:np_
                z[j] = {(:z, j)} ~ Gen.normal(0, 1)
            end
            theta = [0.3 + 0.5 / (1 + exp(-z[j])) for j in 1:np_]      # any smooth positive transform
            zn ~ Gen.normal(0, 1)
            nz = exp(-2.5 + 0.3 * zn) + 1e-5
            xs ~ H.gp_marginal_flat(eng, ops, theta, nz, ts)
        end
        obs = Gen.choicemap((:xs, xs))
        tr, _ = Gen.generate(toy, (ts,), obs)
        sel = Gen.select([(:z, j) for j in 1:np_]..., :zn)
        _, vals, grads = Gen.choice_gradients(tr, sel, nothing)
        # finite differences of the trace score along each selected choice
        for addr in vcat([(:z, j) for j in 1:np_], [:zn])
            v = tr[addr]; h = 1e-6
            tp_, = Gen.update(tr, (ts,), (Gen.NoChange(),), Gen.choicemap((addr, v + h)))
            tm_, = Gen.update(tr, (ts,), (Gen.NoChange(),), Gen.choicemap((addr, v - h)))
            fd = (Gen.get_score(tp_) - Gen.get_score(tm_)) / (2h)
            @test abs(grads[addr] - fd) <= 1e-4 * max(1.0, abs(fd))
        end
        before = H.grad_reuse_stats(eng).reused
        tr2, _ = Gen.hmc(tr, sel; L=5, eps=0.01)
        @test isfinite(Gen.get_score(tr2))
        @test H.grad_reuse_stats(eng).reused > before        # leapfrog: update (value) then choice_gradients at the same point
        # a trace whose xs is NOT the resident series (simulate) is scored by the reference's arithmetic, never against
        # the wrong data
        tr4 = Gen.simulate(toy, (ts,))
        @test isfinite(Gen.get_score(tr4))
        th4 = [0.3 + 0.5 / (1 + exp(-tr4[(:z, j)])) for j in 1:np_]
        nz4 = exp(-2.5 + 0.3 * tr4[:zn]) + 1e-5
        @test relerr(Gen.logpdf(H.gp_marginal_flat, tr4[:xs], eng, ops, th4, nz4, ts),
                     ref_logpdf(H.node_from_flat(ops, th4), nz4, ts, tr4[:xs])) <= 1e-12
    end

    @testset "communicator bookkeeping, explicit wait" begin
        @test H.comm_count(eng) == 0                     # no communicator on a plain single-GPU engine
        @test H.shard_range(11, 1, 2) == 7:11 && H.shard_range(11, 0, 2) == 1:6
        H.wait!(eng)                                     # nothing pending: returns at once, no latched fault
        lw = collect(1.0:5.0)
        @test H.allgather_logweights!(eng, copy(lw)) == lw      # one rank: already complete
    end

    H.destroy!(eng)
end
