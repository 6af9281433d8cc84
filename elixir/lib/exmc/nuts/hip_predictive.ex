defmodule Exmc.NUTS.HipPredictive do
  @moduledoc """
  `Exmc.Predictive.posterior_predictive/3` of a built model kind on the device (DESIGN.md "Posterior
  predictive"): every chain's replicates are drawn by one generator in one kernel launch
  (`Exmc.NUTS.HipPredictiveNative.posterior_predictive/6`), bit-identical to the statement of
  `predictive.ex` and the `sample/2` callbacks it calls.

  The model is a map of `Exmc.NUTS.HipSampler.compile_kind/5` (it carries `{kind, data}`); `trace` is the
  `[chain][draw][dim]` kernel-order binary the sampling functions return (`trace.draws` of
  `sample_chains_vectorized/3`), opts `:num_chains` and `:num_draws`, `:seed` (0) and `:chain_lo` (0: a
  caller that shards its chains offsets the seeds with it). Returns per chain what the reference returns
  for the one trace it is handed: a list of `%{datum_key => Nx.t({num_draws})}`, one map per chain, chain
  c drawn with `seed + 7919 * (chain_lo + c)`; with `num_chains: 1` the map itself. The keys are the
  reference's obs keys where it has them (eight_schools `"y_obs_j"`, simple `{"y_obs", i}`), else
  `{"returns", t}`, `{"y", i}`, `{"radon", i}`, every index 0-based and in the kind's data order
  (`opts[:names]`, a list of N keys, replaces them).

  Deviations from the reference: the unit is the datum of the kind, whatever way the reference writes
  the likelihood node; the datums are walked in the kind's data order, not in map order; a gamma variate
  that rejects 64 times in a row is `:nan` in effect (a NaN in the tensor); generated models raise
  `{:exmc_hip_error, 4, _}`.
  """

  alias Exmc.NUTS.HipPredictiveNative

  def posterior_predictive(%{model: model}, trace, opts \\ []) do
    c = Keyword.fetch!(opts, :num_chains)
    s = Keyword.fetch!(opts, :num_draws)
    yrep = HipPredictiveNative.posterior_predictive(model, trace, c, s, Keyword.get(opts, :seed, 0), Keyword.get(opts, :chain_lo, 0))
    n = div(byte_size(yrep), 8 * c * s)
    names = Keyword.get(opts, :names) || datum_names(elem(model, 0), n)

    maps =
      for ch <- 0..(c - 1) do
        # [draw][datum] of the chain -> one {num_draws} tensor per datum
        t = binary_part(yrep, ch * s * n * 8, s * n * 8) |> Nx.from_binary(:f64) |> Nx.reshape({s, n})
        names |> Enum.with_index() |> Map.new(fn {name, i} -> {name, t[[.., i]]} end)
      end

    if c == 1, do: hd(maps), else: maps
  end

  # the kinds of include/exmc_hip.h: 1 simple, 2 eight_schools, 3 sv, 4 logistic, 5 radon, 7 sv_ncp
  # (Exmc.NUTS.HipLooPit names its datums with it too)
  @doc false
  def datum_names(2, n), do: for(j <- 0..(n - 1), do: "y_obs_#{j}")
  def datum_names(1, n), do: for(i <- 0..(n - 1), do: {"y_obs", i})
  def datum_names(kind, n) when kind in [3, 7], do: for(t <- 0..(n - 1), do: {"returns", t})
  def datum_names(5, n), do: for(i <- 0..(n - 1), do: {"radon", i})
  def datum_names(_kind, n), do: for(i <- 0..(n - 1), do: {"y", i})
end
