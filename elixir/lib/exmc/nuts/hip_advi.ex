defmodule Exmc.NUTS.HipAdvi do
  @moduledoc """
  `Exmc.ADVI.fit/2` on the device (DESIGN.md "ADVI"): the stochastic-gradient loop with its convergence
  test and the draws run in one kernel launch (`Exmc.NUTS.HipAdviNative.fit/12`), bit-identical to the
  statement of `advi.ex` in the lane layout of the launch.

  The model is a map of `Exmc.NUTS.HipSampler.compile_kind/5` (it carries `{kind, data}`, the PointMap and
  the flat order). Returns what `ADVI.fit/2` returns: `{trace, info}` with
  `trace = %{id => Nx.t({num_draws, ...shape})}` in constrained space (`Transform.apply` per PointMap
  entry, as the reference's `build_trace` does) and
  `info = %{elbo_history:, mu:, log_sigma:, converged:, num_iters:}`, `elbo_history` a list of `num_iters`
  floats, `mu` and `log_sigma` flat-order `{d}` tensors in unconstrained space. With `num_fits: n` (n > 1)
  it returns `{[trace], [info], best_fit}`, fit c seeded with `seed + 7919 * c` and `best_fit` the first
  fit of the largest mean ELBO over its last half window; `chain_lo:` offsets the seeds for a caller that
  shards.

  Deviations from the reference: `max_iters >= 1`, `num_draws >= 1`, `num_mc_samples >= 1`,
  `window_size >= 2` (ArgumentError otherwise); where `sum(log_sigma)` is not a number the reference
  raises, here the history carries `:nan` / `:infinity` from there on and the fit does not converge.
  """

  alias Exmc.NUTS.{HipAdviNative, HipSampler}
  alias Exmc.Transform

  @default_opts [
    num_draws: 1000,
    max_iters: 10_000,
    learning_rate: 0.01,
    num_mc_samples: 1,
    seed: 0,
    convergence_tol: 1.0e-4,
    window_size: 100,
    num_fits: 1,
    chain_lo: 0,
    lanes: 0
  ]

  def fit(%{model: model, pm: pm, perm: perm}, opts \\ []) do
    opts = Keyword.merge(@default_opts, opts)
    n = opts[:num_fits]
    s = opts[:num_draws]
    iters = opts[:max_iters]

    if s < 1 or iters < 1 or opts[:num_mc_samples] < 1 or opts[:window_size] < 2 or n < 1 do
      raise ArgumentError, "num_draws >= 1, max_iters >= 1, num_mc_samples >= 1, window_size >= 2, num_fits >= 1"
    end

    {draws, mu, log_sigma, history, num_iters, converged} =
      HipAdviNative.fit(model, perm, n, opts[:chain_lo], s, iters, opts[:num_mc_samples], opts[:window_size],
        opts[:learning_rate] * 1.0, opts[:convergence_tol] * 1.0, opts[:seed], opts[:lanes])

    d = pm.size
    ints = fn bin -> for <<x::signed-32-native <- bin>>, do: x end
    {ns, cs} = {ints.(num_iters), ints.(converged)}

    results =
      for c <- 0..(n - 1) do
        flat = HipSampler.flat_draws(binary_part(draws, c * s * d * 8, s * d * 8), s, d, perm)
        ni = Enum.at(ns, c)

        info = %{
          elbo_history: for(<<x::binary-size(8) <- binary_part(history, c * iters * 8, ni * 8)>>, do: number(x)),
          mu: flat_vec(binary_part(mu, c * d * 8, d * 8), perm),
          log_sigma: flat_vec(binary_part(log_sigma, c * d * 8, d * 8), perm),
          converged: Enum.at(cs, c) == 1,
          num_iters: ni
        }

        {build_trace(flat, pm), info}
      end

    if n == 1 do
      hd(results)
    else
      infos = Enum.map(results, &elem(&1, 1))
      h = div(opts[:window_size], 2)

      # the first fit of the largest mean ELBO over its last half window (nil: none is a number)
      best =
        case infos |> Enum.map(&tail_mean(&1.elbo_history, h)) |> Enum.with_index() |> Enum.filter(&is_float(elem(&1, 0))) do
          [] -> nil
          finite -> finite |> Enum.max_by(&elem(&1, 0)) |> elem(1)
        end

      {Enum.map(results, &elem(&1, 0)), infos, best}
    end
  end

  defp tail_mean(history, h) do
    tail = Enum.take(history, -h)
    if Enum.all?(tail, &is_float/1), do: Enum.sum(tail) / length(tail), else: :nan
  end

  # NaN and the infinities are not Erlang floats
  defp number(<<x::float-64-native>>), do: x
  defp number(<<bits::64-native>>), do: if(Bitwise.band(bits, 0x000FFFFFFFFFFFFF) == 0, do: :infinity, else: :nan)

  defp flat_vec(bin, perm), do: Nx.from_binary(bin, :f64) |> Nx.take(Nx.tensor(perm, type: :s64))

  # advi.ex:175-186
  defp build_trace(flat, pm) do
    num_draws = elem(Nx.shape(flat), 0)

    Map.new(pm.entries, fn entry ->
      sliced = Nx.slice_along_axis(flat, entry.offset, entry.length, axis: 1)
      reshaped = Nx.reshape(sliced, Tuple.insert_at(entry.shape, 0, num_draws))
      {entry.id, Transform.apply(entry.transform, reshaped)}
    end)
  end
end
