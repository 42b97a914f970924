// GPU run of the NodeJS host (tests/test_gpu_fold_in_node.py): warm-starts from the factor files Python wrote into
// <dir>/ml_factors_ready, trains, then answers recommendItemsForRatings and foldIn from the trained handle.
'use strict';
const path = require('path');
const fs = require('fs');
const root = path.join(__dirname, '..', '..', 'you-can-not-recommend_amd');
const Emf = require(path.join(root, 'lib', 'emf', 'Emf'));
const { Dataset } = require(path.join(root, 'lib', 'Dataset'));

const input = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const F = input.useDoublePrecision ? Float64Array : Float32Array;
const t = { user: Int32Array.from(input.user), item: Int32Array.from(input.item), rating: F.from(input.rating) };
const ds = new Dataset(input.users, input.items, t, Int8Array.from(input.type), F);
const lord = Emf.createLord();
lord.init({}, { factorsCount: input.k, trainIters: input.iters, dataDir: input.dir, dbType: 'ml', useDoublePrecision: input.useDoublePrecision,
  ratingsInPortionForRmse: input.rip, numThreadsForTrain: { als: input.threads } });
lord.train(ds).then(() => {
  const recs = lord.recommendItemsForRatings(input.ratings, input.limit, input.minRecommendRating, input.unratedItems);
  const users = lord.foldIn('byUser', input.ratings);
  const item = lord.foldIn('byItem', input.itemRows, input.itemStore);
  const stored = lord.foldIn('byUser', input.ratings.slice(0, 1), input.userStore);
  const after = lord.recommendItemsForUsers(input.userStore, input.limit, input.minRecommendRating);
  // foldIn('byItem') is refused where the user matrix is not replicated on the rank; the user side is not
  let bandsError = null, bandsUsers = null;
  lord.bands = [0, input.users]; lord.options.world = 2;
  try { lord.foldIn('byItem', input.itemRows); } catch (e) { bandsError = e.message; }
  bandsUsers = Array.from(lord.foldIn('byUser', input.ratings).status);
  const arr = (r) => ({ rows: Array.from(r.rows), status: Array.from(r.status) });
  console.log(JSON.stringify({ recs, users: arr(users), item: arr(item), stored: arr(stored), after, bandsError, bandsUsers }));
  lord.destroy();
}).catch((e) => { console.error(e); process.exit(1); });
