defmodule Exmc.NUTS.HipPathfinder do
  @moduledoc """
  `Exmc.Pathfinder.fit/2` on the device (DESIGN.md "Pathfinder"): the seeded start, the L-BFGS path, the
  ELBO of every path point and the draws run in one kernel launch (`Exmc.NUTS.HipPathfinderNative.fit/9`),
  bit-identical to the statement of `pathfinder.ex` in the lane layout of the launch.

  The model is a map of `Exmc.NUTS.HipSampler.compile_kind/5` (it carries `{kind, data}`, the PointMap and
  the flat order). Returns what `Pathfinder.fit/2` returns: `{draws, info}` with
  `draws = %{id => Nx.t({num_draws, ...shape})}` in constrained space (`Transform.apply` per PointMap
  entry, as the reference's `build_trace` does) and `info = %{elbo:, mu:, sigma:, num_iters:}`, `mu` and
  `sigma` as flat-order `{d}` tensors in unconstrained space; `info` also carries `best_index` and
  `status`. With `num_paths: n` (n > 1) it returns `{[draws], [info], best_path}`, path c seeded with
  `seed + 7919 * c`; `chain_lo:` offsets the seeds for a caller that shards.

  Deviations from the reference: `max_iters >= 1`, `num_draws >= 1`, `history_size in 1..6`
  (ArgumentError otherwise); a path with no finite ELBO has `status: 1` and `elbo: :nan` with NaN `mu`,
  `sigma` and draws, where the reference raises.
  """

  alias Exmc.NUTS.{HipPathfinderNative, HipSampler}
  alias Exmc.Transform

  @default_opts [num_draws: 1000, max_iters: 100, history_size: 6, seed: 0, num_paths: 1, chain_lo: 0, lanes: 0]

  def fit(%{model: model, pm: pm, perm: perm}, opts \\ []) do
    opts = Keyword.merge(@default_opts, opts)
    n = opts[:num_paths]
    s = opts[:num_draws]

    if s < 1 or opts[:max_iters] < 1 or opts[:history_size] < 1 or opts[:history_size] > 6 or n < 1 do
      raise ArgumentError, "num_draws >= 1, max_iters >= 1, history_size in 1..6, num_paths >= 1"
    end

    {draws, mu, sigma, elbo, num_iters, best_index, status} =
      HipPathfinderNative.fit(model, perm, n, opts[:chain_lo], s, opts[:max_iters], opts[:history_size],
        opts[:seed], opts[:lanes])

    d = pm.size
    ints = fn bin -> for <<x::signed-32-native <- bin>>, do: x end
    {iters, bests, stats} = {ints.(num_iters), ints.(best_index), ints.(status)}

    results =
      for c <- 0..(n - 1) do
        flat = HipSampler.flat_draws(binary_part(draws, c * s * d * 8, s * d * 8), s, d, perm)

        info = %{
          elbo: number(binary_part(elbo, c * 8, 8)),
          mu: flat_vec(binary_part(mu, c * d * 8, d * 8), perm),
          sigma: flat_vec(binary_part(sigma, c * d * 8, d * 8), perm),
          num_iters: Enum.at(iters, c),
          best_index: Enum.at(bests, c),
          status: Enum.at(stats, c)
        }

        {build_trace(flat, pm), info}
      end

    if n == 1 do
      hd(results)
    else
      infos = Enum.map(results, &elem(&1, 1))

      # the first path of the largest finite ELBO (nil: none is finite)
      best =
        case infos |> Enum.with_index() |> Enum.filter(fn {i, _} -> is_float(i.elbo) end) do
          [] -> nil
          finite -> finite |> Enum.max_by(fn {i, _} -> i.elbo end) |> elem(1)
        end

      {Enum.map(results, &elem(&1, 0)), infos, best}
    end
  end

  # NaN and the infinities are not Erlang floats
  defp number(<<x::float-64-native>>), do: x
  defp number(<<bits::64-native>>), do: if(Bitwise.band(bits, 0x000FFFFFFFFFFFFF) == 0, do: :infinity, else: :nan)

  defp flat_vec(bin, perm), do: Nx.from_binary(bin, :f64) |> Nx.take(Nx.tensor(perm, type: :s64))

  # pathfinder.ex:192-203
  defp build_trace(flat, pm) do
    num_draws = elem(Nx.shape(flat), 0)

    Map.new(pm.entries, fn entry ->
      sliced = Nx.slice_along_axis(flat, entry.offset, entry.length, axis: 1)
      reshaped = Nx.reshape(sliced, Tuple.insert_at(entry.shape, 0, num_draws))
      {entry.id, Transform.apply(entry.transform, reshaped)}
    end)
  end
end
