defmodule Exmc.NUTS.HipPpc do
  @moduledoc """
  Posterior predictive checks of a built model kind on the device (DESIGN.md "Posterior predictive
  checks"): the replicates `Exmc.NUTS.HipPredictive.posterior_predictive/3` would return at the same
  seed, reduced in the kernel that draws them (`Exmc.NUTS.HipPpcNative.ppc/6`), so that a trace of any
  size is checked without its replicate matrix.

  The model is a map of `Exmc.NUTS.HipSampler.compile_kind/5`; `trace` is the `[chain][draw][dim]`
  kernel-order binary the sampling functions return, opts `:num_chains` and `:num_draws`, `:seed` (0)
  and `:chain_lo` (0). Returns

      %{mean: Nx.t({n}), var: Nx.t({n}), p_lt: Nx.t({n}), p_eq: Nx.t({n}), pit: Nx.t({n}),
        t_obs: %{mean: _, var: _, min: _, max: _}, p_value: %{mean: _, var: _, min: _, max: _}}

  per datum in the kind's data order: the replicates' mean and variance, the share of replicates below
  and equal to the observation, `pit = p_lt + 0.5 * p_eq`; per test statistic of the whole data set its
  observed value and the share of replicated data sets at or above it (the Bayesian p-value). Generated
  models raise `{:exmc_hip_error, 4, _}`.
  """

  alias Exmc.NUTS.HipPpcNative

  @stats [:mean, :var, :min, :max]

  def ppc(%{model: model}, trace, opts \\ []) do
    c = Keyword.fetch!(opts, :num_chains)
    s = Keyword.fetch!(opts, :num_draws)
    {datum, t_obs, p_value} = HipPpcNative.ppc(model, trace, c, s, Keyword.get(opts, :seed, 0), Keyword.get(opts, :chain_lo, 0))
    n = div(byte_size(datum), 32)
    t = datum |> Nx.from_binary(:f64) |> Nx.reshape({n, 4})
    p_lt = t[[.., 2]]
    p_eq = t[[.., 3]]

    %{
      mean: t[[.., 0]],
      var: t[[.., 1]],
      p_lt: p_lt,
      p_eq: p_eq,
      pit: Nx.add(p_lt, Nx.multiply(0.5, p_eq)),
      t_obs: by_stat(t_obs),
      p_value: by_stat(p_value)
    }
  end

  defp by_stat(bin) do
    Map.new(Enum.zip(@stats, bin |> Nx.from_binary(:f64) |> Nx.to_flat_list()))
  end
end
